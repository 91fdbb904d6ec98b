// Host-side check that ha_create's late refusals release the handle: two calls that pass every model check and are
// refused by the last two (the pair-face-record capacity: HA_E_MODEL; persistent manifolds asked of the AllegroHand
// family: HA_E_ARG). Both return before the first HIP call, so this runs without a GPU; build it with the host
// AddressSanitizer and LeakSanitizer reports at exit whatever a refusal left behind.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address -I include tools/diag/create_refusals.hip -o /tmp/create_refusals
#define main handarm_main_unused
#include "../../isaacgym-hand-arm_amd/csrc/handarm_hip.hip"
#undef main
#include <cstdio>
#include <cstring>

// a minimal AllegroHand model: one link, one pool object, every hull the same tetrahedron inside its box
static void tiny_model(ha_model_t* m, int n_link_hulls, int n_static) {
    memset(m, 0, sizeof *m);
    m->n_links = 1;
    m->n_dofs = AH_ND;
    m->n_actors = 1;
    m->n_bodies = 2;
    m->body_object0 = 1;
    m->posed_actor = -1;
    m->n_pool = 1;
    m->n_link_hulls = n_link_hulls;
    m->n_hulls = n_link_hulls + 1;
    m->pool_hull[0] = n_link_hulls;
    m->pool_nhull[0] = 1;
    m->n_static = n_static;
    for (int v = 1; v < 4; v++) m->verts[v][v - 1] = 0.1f;
    for (int j = 0; j < 4; j++) {       // face j: the three vertices but j
        m->plane_loop[j] = (3 * j) | (3 << 16);
        for (int t = 0; t < 3; t++) m->loop_v[3 * j + t] = (uint8_t)((j + 1 + t) % 4);
    }
    int ne = 0;
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++) {   // edge (a, b) lies on the two faces that leave out neither end
            int f[2], nf = 0;
            for (int j = 0; j < 4; j++)
                if (j != a && j != b) f[nf++] = j;
            m->edges[ne++] = (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)f[0] << 16) | ((uint32_t)f[1] << 24);
        }
    for (int k = 0; k < m->n_hulls; k++) {
        m->hull_nverts[k] = 4;
        m->hull_nplanes[k] = 4;
        m->hull_nedges[k] = ne;
        const float box[12] = {0.05f, 0.05f, 0.05f, 0.05f, 0.05f, 0.05f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f};
        memcpy(m->hull_obb[k], box, sizeof box);
    }
}

int main() {
    static ha_model_t m;
    static ha_params_t p;
    p.task = HA_TASK_ALLEGRO_HAND;
    p.n_objects = 1;
    p.num_obs = 88;
    p.num_initial_poses = 1;
    ha_handle h = nullptr;
    tiny_model(&m, 1, 0);
    p.pcm_lin_tol = 0.001f;
    printf("persistent manifolds on AllegroHand: %d (HA_E_ARG = %d)\n", ha_create(&m, &p, 4, &h), HA_E_ARG);
    p.pcm_lin_tol = 0.0f;
    // one object, 16 statics: 17 pairs plus 17 per link hull against room for 1106
    tiny_model(&m, HA_PAIRF_LINK_HULLS + 1, HA_MAX_STATIC);
    printf("pairs over the pair-face records:    %d (HA_E_MODEL = %d)\n", ha_create(&m, &p, 4, &h), HA_E_MODEL);
    printf("handle %p, sizeof(ha_handle_s) = %zu\n", (void*)h, sizeof(ha_handle_s));
    fflush(stdout);         // LeakSanitizer's report ends the process without flushing stdio
    return 0;
}
