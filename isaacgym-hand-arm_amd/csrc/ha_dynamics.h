// ha_dynamics.h - forward kinematics, joint-space inertia and velocity-product forces, Cholesky factor and explicit
// M^-1. Second part of ha_physics.h, which includes it after its layouts and wave sums (not a header of its own).
#pragma once

// ----------------------------------------------------------------------------- kinematics
HD void fk(SimCtx& c) {
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int lane = c.lane;
    // lane i owns link i: its model constants and its joint rotation (one sincos per lane) are loaded and
    // computed before the level chain, so each level only waits on its parent's LDS pose
    bool own = lane < c.L;
    int lev = -1, par = 0, d = -1;
    f3 op = mk3(0, 0, 0), ax = mk3(0, 0, 0);
    qf oq = qf{0, 0, 0, 1}, qa = qf{0, 0, 0, 1};
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
    }
    wsync();
    for (int l = 1; l <= m.max_level; l++) {
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
}

struct SInert { float m; f3 h; float J[9]; };

HD void inert_apply(const SInert& I, f3 w, f3 v, f3& n, f3& f) {
    n = mv3(I.J, w) + cross3(I.h, v);
    f = v * I.m - cross3(I.h, w);
}
HD void inert_apply_lds(const float* Ic, f3 w, f3 v, f3& n, f3& f) {
    f3 h = mk3(Ic[1], Ic[2], Ic[3]);
    n = mv3(Ic + 4, w) + cross3(h, v);
    f = v * Ic[0] - cross3(h, w);
}

// joint-space inertia s.M (D x D) and velocity-product forces s.Cb
HD void dynamics(SimCtx& c) {
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int lane = c.lane, D = c.D, L = c.L;
    SInert I;
    bool own = lane < L;
    if (own) {
        int i = lane;
        float R[9], Iw[9];
        qf lq = ldq(s.lq[i]);
        qmat(lq, R);
        f3 cc = ld3(s.lp[i]) + qrot(lq, ld3(m.link_com[i]));
        rart3(R, m.link_inertia[i], Iw);
        float sc = c.dr ? c.dr[HA_DR_LINK_MASS + i] : 1.0f;     // DR: mass and inertia scale together
#pragma unroll
        for (int k = 0; k < 9; k++) Iw[k] = Iw[k] * sc;
        float mm = m.link_mass[i] * sc;
        I.m = mm;
        I.h = cc * mm;
        float ccd = dot3(cc, cc);
        float cv[3] = {cc.x, cc.y, cc.z};
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) I.J[a * 3 + b] = Iw[a * 3 + b] + mm * ((a == b ? ccd : 0.0f) - cv[a] * cv[b]);
        float* ic = s.u.pd.dyn.Ic[i];
        ic[0] = I.m; ic[1] = I.h.x; ic[2] = I.h.y; ic[3] = I.h.z;
#pragma unroll
        for (int k = 0; k < 9; k++) ic[4 + k] = I.J[k];
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < 6; k++) { s.u.pd.Vl[0][k] = 0.f; s.u.pd.dyn.Al[0][k] = 0.f; }
        }
    }
    // zero M
    for (int k = lane; k < D * D; k += 64) s.u.pd.M[k] = 0.0f;
    wsync();
    // twists / bias accelerations, level by level (per-lane link constants and joint axis read once)
    int my_lev = own ? m.link_level[lane] : -1;
    int my_par = own ? m.link_parent[lane] : 0;
    int my_d = own ? m.link_dof[lane] : -1;
    f3 my_sw = mk3(0, 0, 0), my_sv = mk3(0, 0, 0);
    if (my_d >= 0) {
        f3 axd = ld3(s.ax[my_d]), and_ = ld3(s.an[my_d]);
        float qd = s.qd[my_d];
        my_sw = axd * qd;
        my_sv = cross3(and_, axd) * qd;
    }
    for (int lev = 1; lev <= m.max_level; lev++) {
        if (my_lev == lev) {
            int i = lane, par = my_par, d = my_d;
            f3 vw = ld3(&s.u.pd.Vl[par][0]), vv = ld3(&s.u.pd.Vl[par][3]);
            f3 aw = ld3(&s.u.pd.dyn.Al[par][0]), av = ld3(&s.u.pd.dyn.Al[par][3]);
            if (d >= 0) {
                f3 sw = my_sw, sv = my_sv;
                vw = vw + sw;
                vv = vv + sv;
                aw = aw + cross3(vw, sw);
                av = av + (cross3(vw, sv) + cross3(vv, sw));
            }
            st3(&s.u.pd.Vl[i][0], vw); st3(&s.u.pd.Vl[i][3], vv);
            st3(&s.u.pd.dyn.Al[i][0], aw); st3(&s.u.pd.dyn.Al[i][3], av);
        }
        wsync();
    }
    if (own) {
        int i = lane;
        f3 vw = ld3(&s.u.pd.Vl[i][0]), vv = ld3(&s.u.pd.Vl[i][3]);
        f3 aw = ld3(&s.u.pd.dyn.Al[i][0]), av = ld3(&s.u.pd.dyn.Al[i][3]);
        f3 n1, f1, n2, f2;
        inert_apply(I, aw, av, n1, f1);
        inert_apply(I, vw, vv, n2, f2);
        f3 fn = n1 + (cross3(vw, n2) + cross3(vv, f2));
        f3 ff = f1 + cross3(vw, f2);
        // link damping (ha_params_t v10): the wrench cl m v_com, ca I_com w (moment about the world origin) with the
        // momentum (n2, f2) = (I_com w + c x m v_com, m v_com): g = c x m v_com = h x f2 / m
        float cl = c.p->link_lin_damping, ca = c.p->link_ang_damping;
        if (cl != 0.0f || ca != 0.0f) {
            f3 g = I.m > 0.0f ? cross3(I.h, f2) * (1.0f / I.m) : mk3(0, 0, 0);
            fn = fn + ((n2 - g) * ca + g * cl);
            ff = ff + f2 * cl;
        }
        st3(&s.u.pd.dyn.Fl[i][0], fn); st3(&s.u.pd.dyn.Fl[i][3], ff);
    }
    wsync();
    // backward accumulation of forces and composite inertia, deepest level first. Each parent lane gathers
    // its children itself, highest link index first: the oracle's order (it visits links L-1 .. 0 and adds
    // each into its parent), so the float sums round identically. (LDS float atomics from the children
    // would add in whatever order the hardware serialises them.)
    uint32_t chm = 0;                           // this lane's child links (HA_MAX_LINKS = 32)
    for (int j = 1; j < L; j++) chm |= (m.link_parent[j] == lane) ? (1u << j) : 0u;
    for (int lev = m.max_level - 1; lev >= 0; lev--) {
        if (my_lev == lev && chm) {
            float* F = s.u.pd.dyn.Fl[lane];
            float* C = s.u.pd.dyn.Ic[lane];
            float f[6], ic[13];
#pragma unroll
            for (int k = 0; k < 6; k++) f[k] = F[k];
#pragma unroll
            for (int k = 0; k < 13; k++) ic[k] = C[k];
            for (uint32_t mm = chm; mm;) {
                int j = 31 - __clz(mm);
                mm &= ~(1u << j);
#pragma unroll
                for (int k = 0; k < 6; k++) f[k] = f[k] + s.u.pd.dyn.Fl[j][k];
#pragma unroll
                for (int k = 0; k < 13; k++) ic[k] = ic[k] + s.u.pd.dyn.Ic[j][k];
            }
#pragma unroll
            for (int k = 0; k < 6; k++) F[k] = f[k];
#pragma unroll
            for (int k = 0; k < 13; k++) C[k] = ic[k];
        }
        wsync();
    }
    if (lane < D) {
        int i = m.dof_link[lane];
        f3 axd = ld3(s.ax[lane]), and_ = ld3(s.an[lane]);
        s.Cb[lane] = dot3(axd, ld3(&s.u.pd.dyn.Fl[i][0])) + dot3(cross3(and_, axd), ld3(&s.u.pd.dyn.Fl[i][3]));
    }
    for (int k = lane; k < m.n_mpairs; k += 64) {
        int d = m.mpair[k][0], e = m.mpair[k][1];
        int i = m.dof_link[d];
        f3 axd = ld3(s.ax[d]), and_ = ld3(s.an[d]);
        f3 n, f;
        inert_apply_lds(s.u.pd.dyn.Ic[i], axd, cross3(and_, axd), n, f);
        f3 axe = ld3(s.ax[e]), ane = ld3(s.an[e]);
        float val = dot3(axe, n) + dot3(cross3(ane, axe), f);
        if (d == e) val += m.dof_armature[d];
        s.u.pd.M[d * D + e] = val;
        s.u.pd.M[e * D + d] = val;
    }
    wsync();
}


// M^-1 from M in registers, no LDS round trips or barriers (ND = compile-time DOF count):
//   1. Cholesky M = L L^T, left-looking, lane i holds row i of L (row j of L via v_readlane);
//   2. lane j builds column j of L^-1 by forward substitution;
//   3. lane j back-substitutes L^T x = (L^-1 e_j) -> x = column j of M^-1.
// Stored as S[j][i] = x_j[i] (row j of S = column j of M^-1; S is M^-1 up to rounding, not forced
// symmetric). Every use below reads S the same way the oracle does.
template <int ND>
HD void factor_inverse(SimCtx& c) {
    EnvLDS& s = *c.s;
    const int lane = c.lane;
    const float* Mm = s.u.pd.M;
    float a[ND];
#pragma unroll
    for (int k = 0; k < ND; k++) a[k] = (lane < ND && k <= lane) ? Mm[lane * ND + k] : 0.0f;
#pragma unroll
    for (int j = 0; j < ND; j++) {
        float t = a[j];
#pragma unroll
        for (int k = 0; k < j; k++) t = fmaf(-a[k], bcast(a[k], j), t);
        float ljj = sqrtf(fmaxf(bcast(t, j), 1e-30f));
        a[j] = lane == j ? ljj : (lane > j ? t / ljj : a[j]);
    }
    float rl[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) rl[i] = 1.0f / bcast(a[i], i);
    float y[ND];
#pragma unroll
    for (int i = 0; i < ND; i++) {
        float t = 0.0f;
#pragma unroll
        for (int k = 0; k < i; k++) {
            float lik = bcast(a[k], i);
            t = k >= lane ? fmaf(lik, y[k], t) : t;
        }
        y[i] = i == lane ? rl[i] : (i > lane ? -t * rl[i] : 0.0f);
    }
    float x[ND];
#pragma unroll
    for (int i = ND - 1; i >= 0; i--) {
        float t = y[i];
#pragma unroll
        for (int k = i + 1; k < ND; k++) t = fmaf(-bcast(a[i], k), x[k], t);
        x[i] = t * rl[i];
    }
    if (lane < ND) {
#pragma unroll
        for (int i = 0; i < ND; i++) c.Minv[lane * ND + i] = x[i];
    }
    wsync();
}
