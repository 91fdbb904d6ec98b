// ha_cartesian_multi.h - whole-hand Cartesian controller: up to HA_CART_MAX_TASKS links (the flange or palm pose and
// the fingertip positions) stacked into ONE damped least-squares step per env (ha_cartesian_multi_targets of
// include/handarm_abi.h). ha_cartesian.h commands one link per launch; one launch per fingertip would overwrite the
// shared arm DOFs each time, which is no solution of the joint problem.
//
// One wavefront per env, HA_KIN_WAVES envs per workgroup, each with its own LDS block (CartMultiLDS, 9.3 KB) and
// wave-level syncs only, as ha_cartesian_kernel. What differs from it is the linear algebra: stacked, the system
// A = Jw Jw^T + lambda^2 I is up to 24 x 24 and, with more rows than DOFs, singular up to lambda^2, and a float32
// factorisation of it loses the step (up to 6e-3 rad). So J and e stay float32 (FK in float32 is what
// limits them anyway) and everything from A on is float64: the float32 products promote exactly, gfx950 has native
// v_fma_f64, and the system is tiny.
//   1. FK level by level over the UNION of the tasks' base-to-link paths, to the largest depth (one sweep, not one per
//      task); ha_cartesian.h step 1.
//   2. per task t (loop to the launch's T): tool point, task error e_t and the lane's Jacobian column, exactly the
//      single-link kernel's expressions; rows row0[t] .. row0[t] + nrow[t] - 1 (3 for a position-only task, else 6) of
//      J (lane = DOF), e and the row weight w go to LDS UNWEIGHTED. err_out[env][t] = e_t (angular part 0 when
//      position only).
//   3. A[r][c] = w_r w_c sum_d J[r][d] J[c][d] (+ lambda^2 on the diagonal), one lane per entry, 64 entries a pass,
//      float64 fma chains. The weights are applied here, in float64: Jw itself is never rounded.
//   4. A = L D L^T in place, right-looking, lane & 31 = row, one wave sync per column: at column j every lane reads the
//      pivot A[j][j] and takes its reciprocal (the one division per pivot; pivots are >= lambda^2 > 0 because Jw Jw^T
//      is positive semidefinite), row i > j subtracts (A[i][j] / d_j) A[c][j] from A[i][c], c = j+1..i, the wave's two
//      halves taking alternate columns. Column j is only read at step j, so the sync between columns is the only one.
//      No square root: L[i][j] = A[i][j] / d_j is formed where it is used. Lane j keeps 1 / d_j in a register.
//   5. the right-hand sides live one entry per lane (lane = row): b = diag(w) e and, with the posture term,
//      b2 = diag(w) J z. Forward, diagonal and back substitution are column sweeps in which the solved entry of lane j
//      is broadcast with v_readlane (no LDS, no sync); both right-hand sides ride in the same sweep.
//   6. w_r y_r back to LDS, then lane = DOF: dq_d = sum_r J[r][d] (w_r y_r) in float64 (+ z_d - the same with y2).
//   7. step limit on the whole dq, then targets[env][d] = clamp(q_d + dq_d, lower, upper) for d in U, the union of the
//      tasks' selected DOF sets; the sum q + dq is rounded to float32 once. Nothing else of targets is written.
// The early returns of spare waves are legal: waves never meet at a workgroup barrier.
#pragma once
#include "ha_cartesian.h"

#define HA_CM_LD (HA_CART_MAX_ROWS + 1)   // row stride of J and A in LDS: odd, so that a column read spreads over the banks

struct CartMultiLDS {
    double A[HA_CART_MAX_ROWS][HA_CM_LD];  // lower triangle: A, then column by column its L D L^T factor (unscaled columns)
    double y[2][HA_CART_MAX_ROWS];         // w_r y_r of the task solve and of the posture solve
    float lp[HA_MAX_LINKS][3];
    float lq[HA_MAX_LINKS][4];
    float ax[HA_MAX_DOFS][3];              // world joint axis
    float an[HA_MAX_DOFS][3];              // world joint anchor
    float J[HA_CART_MAX_ROWS][HA_CM_LD];   // unweighted rows, lane = DOF
    float e[HA_CART_MAX_ROWS];             // unweighted error rows
    float w[HA_CART_MAX_ROWS];             // row weights
    float z[HA_MAX_DOFS];                  // posture step null_gain (q_rest - q) on U
};

struct CartMultiLaunch {
    const ha_model_t* model;
    const float* dof_state;                // [N][D][2]
    const float* goal;                     // [n][T][7] or [n][T][6], row k for the k-th launched env
    float* targets;                        // [N][D]
    float* err_out;                        // [N][T][6] or null
    const float* q_rest;                   // [D] or null (null_gain == 0)
    const int32_t* env_ids;                // [n] or null
    double lam2;
    int N, n, T, R, depth, mode;
    uint32_t path;                         // union of the tasks' base-to-link paths (bit = link index)
    uint32_t dofs;                         // U: union of the tasks' selected DOF sets
    float max_step, null_gain;
    int link[HA_CART_MAX_TASKS], row0[HA_CART_MAX_TASKS], nrow[HA_CART_MAX_TASKS];
    uint32_t tdofs[HA_CART_MAX_TASKS];     // task t's link's ancestor-or-self DOFs the caller selected
    float off[HA_CART_MAX_TASKS][3], w[HA_CART_MAX_TASKS];
};

// lane src's double (src wave-uniform)
HD double cm_bcast(double x, int src) {
    int lo = __builtin_amdgcn_readlane(__double2loint(x), src);
    int hi = __builtin_amdgcn_readlane(__double2hiint(x), src);
    return __hiloint2double(hi, lo);
}

extern "C" __global__ void __launch_bounds__(64 * HA_KIN_WAVES) ha_cartesian_multi_kernel(CartMultiLaunch a) {
    __shared__ CartMultiLDS lds[HA_KIN_WAVES];
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * HA_KIN_WAVES + (threadIdx.x >> 6);
    if (k >= a.n) return;              // the tail workgroup's spare waves (waves never meet at a workgroup barrier)
    const int env = a.env_ids ? a.env_ids[k] : k;
    if (env < 0 || env >= a.N) return; // a listed index outside the shard is skipped
    CartMultiLDS& s = lds[threadIdx.x >> 6];
    const ha_model_t& m = *a.model;
    const int L = m.n_links, D = m.n_dofs, T = a.T, R = a.R;

    // ---- the lane's joint position, limits and rest position, and the model rows of the links on the tasks' paths
    const bool pose = a.mode == HA_CART_POSE;
    const int gw = pose ? 7 : 6;
    const float* grow = a.goal + (size_t)k * T * gw;
    const bool in = lane < D && ((a.dofs >> lane) & 1u);
    float qd_ = 0.0f, lo = 0.0f, up = 0.0f, z = 0.0f;
    if (lane < D) qd_ = a.dof_state[((size_t)env * D + lane) * 2];
    if (in) {
        lo = m.dof_lower[lane];
        up = m.dof_upper[lane];
        if (a.null_gain > 0.0f) z = a.null_gain * (a.q_rest[lane] - qd_);
    }
    // ---- FK of the links on the union of the paths (ha_cartesian.h, ha_kinematics.h step 1)
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
    if (lane < D) s.z[lane] = z;
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

    // ---- per task: tool point, error (wave-uniform, every lane) and the lane's Jacobian column; rows to LDS
    for (int t = 0; t < T; t++) {
        const int link = a.link[t], r0 = a.row0[t], nr = a.nrow[t];
        const bool ponly = nr == 3;
        const float* g = grow + t * gw;
        const qf ql = ldq(s.lq[link]);
        const f3 pt = ld3(s.lp[link]) + qrot(ql, mk3(a.off[t][0], a.off[t][1], a.off[t][2]));
        float e[6];
        if (pose) {
            f3 dp = ld3(g) - pt;
            e[0] = dp.x; e[1] = dp.y; e[2] = dp.z;
            e[3] = e[4] = e[5] = 0.0f;
            if (!ponly) {              // a position-only task's goal quaternion is not read
                qf qe = qmul(qnormalize(ldq(g + 3)), qf{-ql.x, -ql.y, -ql.z, ql.w});
                if (qe.w < 0.0f) qe = qf{-qe.x, -qe.y, -qe.z, -qe.w};
                f3 v = mk3(qe.x, qe.y, qe.z);
                float vn = sqrtf(fmaf(v.x, v.x, fmaf(v.y, v.y, v.z * v.z)));
                float sc = vn < 1e-6f ? 2.0f : 2.0f * atan2f(vn, qe.w) / vn;
                e[3] = v.x * sc; e[4] = v.y * sc; e[5] = v.z * sc;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; r++) e[r] = g[r];
            e[3] = e[4] = e[5] = 0.0f;
            if (!ponly) {
#pragma unroll
                for (int r = 3; r < 6; r++) e[r] = g[r];
            }
        }
        float jc[6] = {0, 0, 0, 0, 0, 0};
        if (lane < D && ((a.tdofs[t] >> lane) & 1u)) {
            f3 ad = ld3(s.ax[lane]);
            f3 lin = cross3(ad, pt - ld3(s.an[lane]));
            jc[0] = lin.x; jc[1] = lin.y; jc[2] = lin.z;
            jc[3] = ad.x; jc[4] = ad.y; jc[5] = ad.z;
        }
        if (lane < D) {
#pragma unroll
            for (int r = 0; r < 6; r++)
                if (r < nr) s.J[r0 + r][lane] = jc[r];
        }
        if (lane < 6) {
            float v = e[0];
#pragma unroll
            for (int r = 1; r < 6; r++) v = lane == r ? e[r] : v;
            if (lane < nr) {
                s.e[r0 + lane] = v;
                s.w[r0 + lane] = a.w[t];
            }
            if (a.err_out) a.err_out[((size_t)env * T + t) * 6 + lane] = v;
        }
    }
    wsync();

    // ---- A = diag(w) J J^T diag(w) + lambda^2 I in float64, one lane per entry of the lower triangle's square
    for (int idx = lane; idx < R * R; idx += 64) {
        const int r = idx / R, c = idx - r * R;
        if (c <= r) {
            double acc = 0.0;
#pragma unroll 4
            for (int dd = 0; dd < D; dd++) acc = fma((double)s.J[r][dd], (double)s.J[c][dd], acc);
            acc = acc * ((double)s.w[r] * (double)s.w[c]);
            s.A[r][c] = r == c ? acc + a.lam2 : acc;
        }
    }
    // the right-hand sides, lane = row: b = w e, b2 = w (J z)
    const bool row = lane < R;
    const bool posture = a.null_gain > 0.0f;
    double b = 0.0, b2 = 0.0, wr = 0.0;
    if (row) {
        wr = (double)s.w[lane];
        b = wr * (double)s.e[lane];
        if (posture) {
            double acc = 0.0;
#pragma unroll 4
            for (int dd = 0; dd < D; dd++) acc = fma((double)s.J[lane][dd], (double)s.z[dd], acc);
            b2 = wr * acc;
        }
    }
    wsync();

    // ---- A = L D L^T, right-looking; L[i][j] = A[i][j] dinv_j with dinv_j kept by lane j. Row i = lane & 31, and the
    // two halves of the wave share a row's columns by parity (half h takes c = j+1+h, j+3+h, ...), four columns at a
    // time with their loads ahead of their stores: the updates of one step are independent, and the chain of LDS
    // round trips is what the factorisation costs
    const int ri = lane & 31, half = lane >> 5;
    double dinv = 0.0;
    for (int j = 0; j < R; j++) {
        const double rj = 1.0 / s.A[j][j];     // one division per pivot
        if (lane == j) dinv = rj;
        if (ri < R && ri > j) {
            const double lij = -(s.A[ri][j] * rj);
            int c = j + 1 + half;
            for (; c + 6 <= ri; c += 8) {
                const double v0 = s.A[c][j], v1 = s.A[c + 2][j], v2 = s.A[c + 4][j], v3 = s.A[c + 6][j];
                const double a0 = s.A[ri][c], a1 = s.A[ri][c + 2], a2 = s.A[ri][c + 4], a3 = s.A[ri][c + 6];
                s.A[ri][c] = fma(lij, v0, a0);
                s.A[ri][c + 2] = fma(lij, v1, a1);
                s.A[ri][c + 4] = fma(lij, v2, a2);
                s.A[ri][c + 6] = fma(lij, v3, a3);
            }
            for (; c <= ri; c += 2) s.A[ri][c] = fma(lij, s.A[c][j], s.A[ri][c]);
        }
        wsync();
    }

    // ---- L u = b (lane j's entry is final when the sweep reaches column j), v = D^-1 u, L^T y = v
    for (int j = 0; j < R - 1; j++) {
        const double rj = cm_bcast(dinv, j), uj = cm_bcast(b, j), uj2 = cm_bcast(b2, j);
        if (row && lane > j) {
            const double lij = s.A[lane][j] * rj;
            b = fma(-lij, uj, b);
            if (posture) b2 = fma(-lij, uj2, b2);
        }
    }
    b = b * dinv;
    b2 = b2 * dinv;
    for (int j = R - 1; j > 0; j--) {
        const double yj = cm_bcast(b, j), yj2 = cm_bcast(b2, j);
        if (lane < j) {
            const double lji = s.A[j][lane] * dinv;    // L[j][lane]
            b = fma(-lji, yj, b);
            if (posture) b2 = fma(-lji, yj2, b2);
        }
    }
    if (row) {
        s.y[0][lane] = wr * b;
        s.y[1][lane] = wr * b2;
    }
    wsync();

    // ---- dq = Jw^T y (+ z - Jw^T y2), lane = DOF, float64
    double dq = 0.0;
    if (in) {
#pragma unroll 4
        for (int r = 0; r < R; r++) dq = fma((double)s.J[r][lane], s.y[0][r], dq);
        if (posture) {
            double jy = 0.0;
#pragma unroll 4
            for (int r = 0; r < R; r++) jy = fma((double)s.J[r][lane], s.y[1][r], jy);
            dq = dq + ((double)z - jy);
        }
    }
    if (a.max_step > 0.0f) {
        float mx = wave_max(fabsf((float)dq));     // dq is 0 in the lanes outside U
        if (mx > a.max_step) dq = dq * ((double)a.max_step / (double)mx);
    }
    if (in) a.targets[(size_t)env * D + lane] = fminf(fmaxf((float)((double)qd_ + dq), lo), up);
}
