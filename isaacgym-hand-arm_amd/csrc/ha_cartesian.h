// ha_cartesian.h - Cartesian arm controller: one damped least-squares IK step per env, from the bound dof_state to joint
// position targets (ha_cartesian_targets of include/handarm_abi.h). No Isaac Gym counterpart: there the user composes it
// in torch on the Jacobian tensor (refresh, slice, bmm, solve, bmm, add: about ten launches); here it is one launch that
// never stores the Jacobian.
//
// One wavefront per env, HA_KIN_WAVES envs per workgroup, each with its own small LDS block (CartLDS, 2.2 KB: link
// poses, joint axes and anchors, the 6 x D Jacobian, A), the layout of ha_kinematics_kernel. The step kernels' EnvLDS
// is not used: this kernel shares only ha_device.h's math with them and touches none of their state.
//   1. FK level by level, as ha_kinematics.h step 1, restated here and cut down to the links on the path from the base
//      to the controlled link and to that link's depth. The ancestor-DOF mask of the link comes from the host (it has
//      the model), already ANDed with the caller's dof_mask: `dofs`.
//   2. tool point p_t = p_link + R_link offset, and the link's world quaternion.
//   3. task error e: HA_CART_POSE e[0:3] = goal_pos - p_t, e[3:6] the rotation vector of q_goal (normalised) x
//      conj(q_link), shortest arc; HA_CART_DELTA e = goal. position_only zeroes e[3:6] and rows 3..5 of J.
//   4. J (6 x D) in LDS, lane = DOF: column d = (a_d x (p_t - o_d), a_d) for d in `dofs`, else 0.
//   5. A = J J^T + lambda^2 I, one lane per entry; its Cholesky factor and the triangular solves run redundantly in
//      every lane on the same 36 floats (no cross-lane traffic). Pivots are >= lambda^2 > 0: J J^T is positive
//      semidefinite. One division per pivot: its reciprocal multiplies the factor's column and both solves.
//   6. y = A^-1 e, dq_d = sum_r J[r][d] y_r.
//   7. posture term (null_gain > 0): z_d = null_gain (q_rest[d] - q_d) for d in `dofs`, w = J z, y2 = A^-1 w,
//      dq_d += z_d - sum_r J[r][d] y2_r. That is (I - J^T A^-1 J) z, the DAMPED null-space projector: it is not an exact
//      projector, J (I - J^T A^-1 J) z = lambda^2 A^-1 J z is what it leaks into task space. A closed loop with the
//      posture term on therefore settles where the task step and that leak balance, for the AllegroKuka arm at
//      lambda = 0.05, null_gain = 0.5 some 1-4 mm and up to 1e-3 rad from the goal (float64 reference,
//      tests/cartesian_ref.py), not on it.
//   8. step limit (max_step > 0): the whole dq scaled by max_step / max_d |dq_d| when that maximum exceeds max_step (the
//      direction is kept).
//   9. targets[env][d] = clamp(q_d + dq_d, dof_lower[d], dof_upper[d]) for d in `dofs`; no other element of targets is
//      written. err_out[env][0:6] = e when given.
// Dot products are explicit fmaf chains (the build has -ffp-contract=off).
#pragma once
#include "ha_device.h"
#include "../../include/handarm_abi.h"

#ifndef HA_KIN_WAVES
#define HA_KIN_WAVES 4
#endif

struct CartLDS {
    float lp[HA_MAX_LINKS][3];
    float lq[HA_MAX_LINKS][4];
    float ax[HA_MAX_DOFS][3];          // world joint axis
    float an[HA_MAX_DOFS][3];          // world joint anchor
    float J[6][HA_MAX_DOFS];
    float A[36];
};

struct CartLaunch {
    const ha_model_t* model;
    const float* dof_state;            // [N][D][2]
    const float* goal;                 // [n][7] or [n][6], row k for the k-th launched env
    float* targets;                    // [N][D]
    float* err_out;                    // [N][6] or null
    const float* q_rest;               // [D] or null (null_gain == 0)
    const int32_t* env_ids;            // [n] or null
    int N, n, link, depth, mode, position_only;
    uint32_t path;                     // the links from the base to `link` (bit = link index)
    uint32_t dofs;                     // the link's ancestor-or-self DOFs the caller selected
    float off[3], lam2, max_step, null_gain;
};

// wave sum of x (every lane's value; lane 63's DPP result read back, wave-uniform)
HD float cart_sum(float x) {
    x = x + dpp_f<0xB1>(x);
    x = x + dpp_f<0x4E>(x);
    x = x + dpp_f<0x141>(x);
    x = x + dpp_f<0x140>(x);
    return rows_sum(x);
}

// x = A^-1 b for the Cholesky factor G (lower, row-major 6 x 6) of A, whose diagonal holds the RECIPROCALS of the
// pivots: G y = b, then G^T x = y
HD void cart_solve(const float G[36], const float b[6], float x[6]) {
    float y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        float acc = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) acc = fmaf(-G[i * 6 + k], y[k], acc);
        y[i] = acc * G[i * 6 + i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        float acc = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) acc = fmaf(-G[k * 6 + i], x[k], acc);
        x[i] = acc * G[i * 6 + i];
    }
}

extern "C" __global__ void __launch_bounds__(64 * HA_KIN_WAVES) ha_cartesian_kernel(CartLaunch a) {
    __shared__ CartLDS lds[HA_KIN_WAVES];
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * HA_KIN_WAVES + (threadIdx.x >> 6);
    if (k >= a.n) return;              // the tail workgroup's spare waves (waves never meet at a workgroup barrier)
    const int env = a.env_ids ? a.env_ids[k] : k;
    if (env < 0 || env >= a.N) return; // a listed index outside the shard is skipped
    CartLDS& s = lds[threadIdx.x >> 6];
    const ha_model_t& m = *a.model;
    const int L = m.n_links, D = m.n_dofs;

    // ---- every global load of the wave up front, so that their latencies overlap: the goal row, the lane's joint
    // position, limits and rest position, and the model rows of the links on the path to a.link
    const bool pose = a.mode == HA_CART_POSE;
    const float* grow = a.goal + (size_t)k * (pose ? 7 : 6);
    float g[7];
#pragma unroll
    for (int r = 0; r < 6; r++) g[r] = grow[r];
    g[6] = pose ? grow[6] : 1.0f;
    const bool in = lane < D && ((a.dofs >> lane) & 1u);
    float qd_ = 0.0f, lo = 0.0f, up = 0.0f, qr = 0.0f;   // lane d's joint position, limits, rest position
    if (lane < D) qd_ = a.dof_state[((size_t)env * D + lane) * 2];
    if (in) {
        lo = m.dof_lower[lane];
        up = m.dof_upper[lane];
        if (a.q_rest) qr = a.q_rest[lane];
    }
    // ---- FK of the links on the path to a.link (ha_kinematics.h step 1, ha_dynamics.h fk())
    const bool own = lane < L && ((a.path >> lane) & 1u);
    int lev = -1, par = 0, d = -1;
    f3 op = mk3(0, 0, 0), ax = mk3(0, 0, 0);
    qf oq = qf{0, 0, 0, 1}, qa = qf{0, 0, 0, 1};
    if (own) {
        lev = m.link_level[lane];
        par = m.link_parent[lane];
        d = m.link_dof[lane];
        d = d < D ? d : -1;            // d indexes dof_state below: a DOF the model does not have counts as a fixed joint
        op = ld3(m.link_origin_pos[lane]);
        oq = ldq(m.link_origin_quat[lane]);
        ax = ld3(m.link_axis[lane]);
        if (d >= 0) qa = qaxis(ax, a.dof_state[((size_t)env * D + d) * 2]);
    }
    if (lane == 0) {
        st3(s.lp[0], ld3(m.base_pos));
        stq(s.lq[0], ldq(m.base_quat));
    }
    wsync();
    for (int l = 1; l <= a.depth; l++) {
        if (lev == l) {
            qf pq = ldq(s.lq[par]);
            f3 p = ld3(s.lp[par]) + qrot(pq, op);
            qf r = qmul(pq, oq);
            if (d >= 0) {
                r = qmul(r, qa);
                st3(s.ax[d], qrot(r, ax));
                st3(s.an[d], p);
            }
            st3(s.lp[lane], p);
            stq(s.lq[lane], r);
        }
        wsync();
    }

    // ---- tool point and task error (wave-uniform, every lane)
    const qf ql = ldq(s.lq[a.link]);
    const f3 pt = ld3(s.lp[a.link]) + qrot(ql, mk3(a.off[0], a.off[1], a.off[2]));
    float e[6];
    if (pose) {
        f3 dp = ld3(g) - pt;
        qf qe = qmul(qnormalize(ldq(g + 3)), qf{-ql.x, -ql.y, -ql.z, ql.w});
        if (qe.w < 0.0f) qe = qf{-qe.x, -qe.y, -qe.z, -qe.w};
        f3 v = mk3(qe.x, qe.y, qe.z);
        float vn = sqrtf(fmaf(v.x, v.x, fmaf(v.y, v.y, v.z * v.z)));
        float sc = vn < 1e-6f ? 2.0f : 2.0f * atan2f(vn, qe.w) / vn;
        e[0] = dp.x; e[1] = dp.y; e[2] = dp.z;
        e[3] = v.x * sc; e[4] = v.y * sc; e[5] = v.z * sc;
    } else {
#pragma unroll
        for (int r = 0; r < 6; r++) e[r] = g[r];
    }
    if (a.position_only) e[3] = e[4] = e[5] = 0.0f;

    // ---- J, lane = DOF (registers and LDS), then A = J J^T + lambda^2 I, lane = entry
    float jc[6] = {0, 0, 0, 0, 0, 0};
    if (in) {
        f3 ad = ld3(s.ax[lane]);
        f3 lin = cross3(ad, pt - ld3(s.an[lane]));
        jc[0] = lin.x; jc[1] = lin.y; jc[2] = lin.z;
        if (!a.position_only) { jc[3] = ad.x; jc[4] = ad.y; jc[5] = ad.z; }
    }
    if (lane < D) {
#pragma unroll
        for (int r = 0; r < 6; r++) s.J[r][lane] = jc[r];
    }
    wsync();
    if (lane < 36) {
        int r = lane / 6, c = lane - 6 * r;
        float acc = 0.0f;
        for (int dd = 0; dd < D; dd++) acc = fmaf(s.J[r][dd], s.J[c][dd], acc);
        s.A[lane] = r == c ? acc + a.lam2 : acc;
    }
    wsync();
    // Cholesky A = G G^T in every lane (lower triangle of G, 1 / pivot on its diagonal; the upper stays unread)
    float G[36];
#pragma unroll
    for (int t = 0; t < 36; t++) G[t] = s.A[t];
#pragma unroll
    for (int j = 0; j < 6; j++) {
        float dg = G[j * 6 + j];
#pragma unroll
        for (int c = 0; c < j; c++) dg = fmaf(-G[j * 6 + c], G[j * 6 + c], dg);
        dg = 1.0f / sqrtf(dg);         // one division per pivot: the column and both solves multiply by it
        G[j * 6 + j] = dg;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            float v = G[i * 6 + j];
#pragma unroll
            for (int c = 0; c < j; c++) v = fmaf(-G[i * 6 + c], G[j * 6 + c], v);
            G[i * 6 + j] = v * dg;
        }
    }

    // ---- dq = J^T A^-1 e (+ the damped null-space posture term)
    float y[6];
    cart_solve(G, e, y);
    float dq = 0.0f;
#pragma unroll
    for (int r = 0; r < 6; r++) dq = fmaf(jc[r], y[r], dq);
    if (a.null_gain > 0.0f) {
        float z = in ? a.null_gain * (qr - qd_) : 0.0f;
        float w[6], y2[6];
#pragma unroll
        for (int r = 0; r < 6; r++) w[r] = cart_sum(jc[r] * z);
        cart_solve(G, w, y2);
        float jy = 0.0f;
#pragma unroll
        for (int r = 0; r < 6; r++) jy = fmaf(jc[r], y2[r], jy);
        dq = dq + (z - jy);
    }
    if (a.max_step > 0.0f) {
        float mx = wave_max(fabsf(dq));        // dq is 0 in the lanes outside `dofs`
        if (mx > a.max_step) dq = dq * (a.max_step / mx);
    }
    if (in) a.targets[(size_t)env * D + lane] = fminf(fmaxf(qd_ + dq, lo), up);
    if (a.err_out && lane < 6) {
        float v = e[0];
#pragma unroll
        for (int r = 1; r < 6; r++) v = lane == r ? e[r] : v;
        a.err_out[(size_t)env * 6 + lane] = v;
    }
}
