/* ha_cam_hulls.h - the size of the camera ray cast's per-env hull table (csrc/ha_camera.h: CamHullLDS hl[]), on the
 * host: plain C, no HIP dependency, so ha_create (csrc/handarm_hip.hip) and the C oracle library
 * (oracle/physics_oracle.c hao_cam_hull_count, for the CPU tests) compile the same text.
 *
 * An env's table holds every robot link hull, every convex piece of each of its n_obj objects and every static box.
 * The objects of an env are n_obj entries of the pool (object_indices), so the most entries any env can need is the
 * link hulls + the n_obj largest pool_nhull + the statics. ha_render_camera refuses a model whose worst case exceeds
 * HA_CAM_MAX_HULLS: the check is the only thing between a larger model and a write past hl[].
 */
#ifndef HA_CAM_HULLS_H
#define HA_CAM_HULLS_H

#include "handarm_abi.h"

#define HA_CAM_MAX_HULLS (HA_MAX_HULLS + 1)

/* worst-case hull-table entries of one env; -1 when a count is out of the ABI's range */
static inline int ha_cam_hull_count(int n_link_hulls, int n_static, int n_pool, const int32_t* pool_nhull, int n_obj) {
    if (n_link_hulls < 0 || n_static < 0 || n_pool < 0 || n_pool > HA_MAX_POOL || n_obj < 0) return -1;
    int nh[HA_MAX_POOL];
    long long pieces = 0;
    for (int i = 0; i < n_pool; i++) {
        if (pool_nhull[i] < 0) return -1;
        nh[i] = pool_nhull[i];
    }
    /* the n_obj largest, each pool entry once: an env's objects are distinct pool entries (the reference draws them
       with random.sample, multi_object.py:569) */
    for (int o = 0; o < n_obj; o++) {
        int bi = -1;
        for (int i = 0; i < n_pool; i++)
            if (nh[i] > 0 && (bi < 0 || nh[i] > nh[bi])) bi = i;
        if (bi < 0) break;
        pieces += nh[bi];
        nh[bi] = 0;
    }
    long long total = (long long)n_link_hulls + pieces + n_static;
    return total > 0x7fffffffLL ? -1 : (int)total;
}

#endif
