// ha_kinematics.h - link Jacobians and the joint-space inertia as tensors (gym.acquire_jacobian_tensor /
// acquire_mass_matrix_tensor + their refresh calls; ha_refresh_kinematics of include/handarm_abi.h).
//
// One wavefront per env, HA_KIN_WAVES envs per workgroup, each with its own small LDS block (KinLDS, 6.3 KB: link
// poses, joint axes and anchors, the per-link inertias, one buffer for a Jacobian chunk / M). The step kernels' EnvLDS
// is not used: this kernel shares only ha_device.h's math with them and touches none of their state.
//   1. FK level by level, as ha_dynamics.h fk(); on the way down each link also ORs its DOF into its parent's
//      ancestor-DOF mask (<= 24 bits).
//   2. Jacobian [K][6][D], HA_KIN_CHUNK links at a time: one lane per (link, DOF) column computes its six entries,
//      (a_d x (p_i - o_d), a_d) when d is in i's mask, else 0, into the LDS buffer; the chunk (contiguous in the tensor)
//      is then streamed out through its flat (link, row, dof) index, consecutive lanes on consecutive floats, 256 bytes
//      per wave store. Zeros are stored too: the caller never clears the tensor.
//   3. M by composite bodies about the joint anchors. Lane d sums the links DOF d moves (ascending) into the composite's
//      first moment h and inertia J about the anchor o_d; a unit velocity of d gives the composite the momentum
//      f = a_d x h, n = J a_d (about o_d), and M[d][e] = a_e . (n + (o_d - o_e) x f) for every ancestor-or-self DOF e,
//      stored to both triangles (exactly symmetric), dof_armature added on the diagonal, 0 for unrelated DOFs.
//      dynamics() takes its composites about the world origin, where a finger link's own inertia is the small
//      difference of metre-sized terms; about o_d every term has the subtree's own size. Link mass
//      and inertia carry the env's dr_scale[HA_DR_LINK_MASS + i] as in dynamics(). M is staged in the LDS buffer and
//      streamed out like a Jacobian chunk.
#pragma once
#include "ha_device.h"
#include "../../include/handarm_abi.h"

#define HA_KIN_WAVES 4
#define HA_KIN_CHUNK 4          // links per Jacobian chunk: 4 * 6 * HA_MAX_DOFS floats = the size of M

struct KinLDS {
    float lp[HA_MAX_LINKS][3];
    float lq[HA_MAX_LINKS][4];
    float ax[HA_MAX_DOFS][3];          // world joint axis
    float an[HA_MAX_DOFS][3];          // world joint anchor
    float q[HA_MAX_DOFS];
    float bi[HA_MAX_LINKS][13];        // per link: mass, world COM[3], world inertia about the COM[9]
    float fn[HA_MAX_DOFS][6];          // per DOF: its composite's momentum per unit joint velocity, f[3], n[3] about o_d
    float buf[HA_MAX_DOFS * HA_MAX_DOFS];      // a Jacobian chunk, then M
    uint32_t anc[HA_MAX_LINKS];        // link -> its ancestor-or-self DOFs
    int32_t dl[HA_MAX_DOFS];           // DOF -> its link
    int32_t sel[HA_MAX_LINKS];         // the launch's selected links
};
static_assert(HA_KIN_CHUNK * 6 <= HA_MAX_DOFS, "a Jacobian chunk must fit the M buffer");

struct KinLaunch {
    const ha_model_t* model;
    const float* dof_state;            // [N][D][2]
    const float* dr_scale;             // [N][HA_DR_SIZE] when dr_enable, else null
    float* jac;                        // [N][K][6][D] or null
    float* mm;                         // [N][D][D] or null
    const int32_t* links;              // [K] or null (links 1..L-1)
    int N, K;
};

extern "C" __global__ void __launch_bounds__(64 * HA_KIN_WAVES) ha_kinematics_kernel(KinLaunch a) {
    __shared__ KinLDS lds[HA_KIN_WAVES];
    const int lane = threadIdx.x & 63;
    const int env = blockIdx.x * HA_KIN_WAVES + (threadIdx.x >> 6);
    if (env >= a.N) return;            // the tail workgroup's spare waves (waves never meet at a workgroup barrier)
    KinLDS& s = lds[threadIdx.x >> 6];
    const ha_model_t& m = *a.model;
    const int L = m.n_links, D = m.n_dofs, K = a.K;

    // ---- FK (ha_dynamics.h fk()) and the ancestor-DOF masks
    bool own = lane < L;
    int lev = -1, par = 0, d = -1;
    f3 op = mk3(0, 0, 0), ax = mk3(0, 0, 0);
    qf oq = qf{0, 0, 0, 1}, qa = qf{0, 0, 0, 1};
    if (lane < D) {
        s.q[lane] = a.dof_state[((size_t)env * D + lane) * 2];
        s.dl[lane] = 0;
    }
    if (lane < K) {
        // device-resident link indices are range-checked: an invalid one selects the base link (all-zero rows)
        int l = a.links ? a.links[lane] : lane + 1;
        s.sel[lane] = (l >= 1 && l < L) ? l : 0;
    }
    wsync();
    if (own) {
        lev = m.link_level[lane];
        par = m.link_parent[lane];
        d = m.link_dof[lane];
        op = ld3(m.link_origin_pos[lane]);
        oq = ldq(m.link_origin_quat[lane]);
        if (d >= 0) {
            ax = ld3(m.link_axis[lane]);
            qa = qaxis(ax, s.q[d]);
        }
    }
    if (lane == 0) {
        st3(s.lp[0], ld3(m.base_pos));
        stq(s.lq[0], ldq(m.base_quat));
        s.anc[0] = 0u;
    }
    wsync();
    for (int l = 1; l <= m.max_level; l++) {
        if (lev == l) {
            qf pq = ldq(s.lq[par]);
            f3 p = ld3(s.lp[par]) + qrot(pq, op);
            qf r = qmul(pq, oq);
            uint32_t am = s.anc[par];
            if (d >= 0) {
                r = qmul(r, qa);
                st3(s.ax[d], qrot(r, ax));
                st3(s.an[d], p);
                s.dl[d] = lane;
                am |= 1u << d;
            }
            st3(s.lp[lane], p);
            stq(s.lq[lane], r);
            s.anc[lane] = am;
        }
        wsync();
    }

    // ---- Jacobian, a chunk of links at a time: columns into LDS, then the chunk's floats in tensor order
    if (a.jac) {
        float* out = a.jac + (size_t)env * K * 6 * D;
        for (int k0 = 0; k0 < K; k0 += HA_KIN_CHUNK) {
            const int nk = K - k0 < HA_KIN_CHUNK ? K - k0 : HA_KIN_CHUNK;
            for (int p = lane; p < nk * D; p += 64) {
                int kk = p / D, dd = p - kk * D;
                int i = s.sel[k0 + kk];
                f3 lin = mk3(0, 0, 0), ang = mk3(0, 0, 0);
                if ((s.anc[i] >> dd) & 1u) {
                    ang = ld3(s.ax[dd]);
                    lin = cross3(ang, ld3(s.lp[i]) - ld3(s.an[dd]));
                }
                float* c = s.buf + kk * 6 * D + dd;
                c[0] = lin.x; c[D] = lin.y; c[2 * D] = lin.z;
                c[3 * D] = ang.x; c[4 * D] = ang.y; c[5 * D] = ang.z;
            }
            wsync();
            float* o = out + k0 * 6 * D;
            for (int f = lane; f < nk * 6 * D; f += 64) o[f] = s.buf[f];
            wsync();
        }
    }
    if (!a.mm) return;

    // ---- per-link inertia in the world frame (as dynamics(): DR scales mass and inertia together)
    if (own) {
        float R[9], Iw[9];
        qf lq = ldq(s.lq[lane]);
        qmat(lq, R);
        f3 cc = ld3(s.lp[lane]) + qrot(lq, ld3(m.link_com[lane]));
        rart3(R, m.link_inertia[lane], Iw);
        float sc = a.dr_scale ? a.dr_scale[(size_t)env * HA_DR_SIZE + HA_DR_LINK_MASS + lane] : 1.0f;
        float* b = s.bi[lane];
        b[0] = m.link_mass[lane] * sc;
        st3(b + 1, cc);
#pragma unroll
        for (int k = 0; k < 9; k++) b[4 + k] = Iw[k] * sc;
    }
    wsync();
    // ---- composite of the links DOF `lane` moves, about its anchor, and its momentum per unit joint velocity
    if (lane < D) {
        f3 ad = ld3(s.ax[lane]), od = ld3(s.an[lane]);
        f3 h = mk3(0, 0, 0);
        float J[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 1; i < L; i++) {
            if (!((s.anc[i] >> lane) & 1u)) continue;
            const float* b = s.bi[i];
            float mi = b[0];
            f3 r = ld3(b + 1) - od;
            h = h + r * mi;
            float rr = dot3(r, r);
            float rv[3] = {r.x, r.y, r.z};
#pragma unroll
            for (int u = 0; u < 3; u++)
#pragma unroll
                for (int v = 0; v < 3; v++) J[u * 3 + v] = J[u * 3 + v] + (b[4 + u * 3 + v] + mi * ((u == v ? rr : 0.0f) - rv[u] * rv[v]));
        }
        st3(&s.fn[lane][0], cross3(ad, h));
        st3(&s.fn[lane][3], mv3(J, ad));
    }
    wsync();
    for (int t = lane; t < D * D; t += 64) {
        int x = t / D, y = t - x * D;
        if (y > x) continue;
        // the deeper DOF of the pair carries the composite; unrelated DOFs do not couple
        int dd = -1, e = -1;
        if ((s.anc[s.dl[x]] >> y) & 1u) { dd = x; e = y; }
        else if ((s.anc[s.dl[y]] >> x) & 1u) { dd = y; e = x; }
        float val = 0.0f;
        if (dd >= 0) {
            f3 f = ld3(&s.fn[dd][0]), n = ld3(&s.fn[dd][3]);
            val = dot3(ld3(s.ax[e]), n + cross3(ld3(s.an[dd]) - ld3(s.an[e]), f));
            if (x == y) val = val + m.dof_armature[x];
        }
        s.buf[x * D + y] = val;
        s.buf[y * D + x] = val;
    }
    wsync();
    float* mo = a.mm + (size_t)env * D * D;
    for (int t = lane; t < D * D; t += 64) mo[t] = s.buf[t];
}
