// ha_solve.h - constraint rows, projected Gauss-Seidel, forces and integration: substep(). Last part of ha_physics.h,
// which includes it after ha_collide.h (not a header of its own).
#pragma once

// ----------------------------------------------------------------------------- constraint rows
// Jacobian of body `body` (an object: 0 <= body < 100) into the object blocks Job of a compact row (slot so0 -> 0,
// else 1; Job = J + D for a dense row). A link's robot block comes from the link's DOF mask instead of a walk up the
// link tree (substep, link_dof_masks; the comparison is in profiles/r07_kuka_rows_pgs.txt)
HD void jac_obj(const SimCtx& c, int body, f3 x, f3 dir, float sgn, float* Job, int so0) {
    if (body < 0 || body >= 100) return;
    f3 r = x - ld3(c.o[body].oc);
    f3 ang = cross3(r, dir);
    float* Jo = Job + (body == so0 ? 0 : 6);
    Jo[0] += sgn * dir.x; Jo[1] += sgn * dir.y; Jo[2] += sgn * dir.z;
    Jo[3] += sgn * ang.x; Jo[4] += sgn * ang.y; Jo[5] += sgn * ang.z;
}

// Lane = link: the DOFs on the link's path to the root (its own included), a bit each. One coalesced load of the
// link's parent and DOF, then pointer jumping in registers: after round k a lane holds the DOFs of its 2^k nearest
// ancestors-or-self and `par` is the link 2^k above (-1: past the root), so five rounds cover any tree of
// HA_MAX_LINKS links. Needs every lane active (ds_bpermute reads 0 from a disabled lane).
HD uint32_t link_dof_masks(const SimCtx& c) {
    static_assert(HA_MAX_LINKS <= 32 && HA_MAX_DOFS <= 32, "five jumps; a 32-bit DOF mask");
    int lane = c.lane, par = -1, d = -1;
    if (lane < c.L) {
        par = c.m->link_parent[lane];
        d = c.m->link_dof[lane];
    }
    uint32_t am = d >= 0 ? 1u << d : 0u;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        int src = par < 0 ? lane : par;
        uint32_t pm = (uint32_t)lane_read_i((int)am, src);
        int pp = lane_read_i(par, src);
        if (par >= 0) {
            am |= pm;
            par = pp;
        }
    }
    return am;
}

HD void tangents(f3 n, f3& t1, f3& t2) {
    f3 a = fabsf(n.x) < 0.9f ? mk3(1, 0, 0) : mk3(0, 1, 0);
    f3 t = cross3(n, a);
    float l = sqrtf(dot3(t, t));
    t1 = t * (1.0f / l);
    t2 = cross3(n, t1);
}

// Object blocks of one contact row (slot 0: object so0, slot 1: so1; row direction dir), in registers, by the
// expressions of oracle/physics_oracle.c:jac_body and the stored rows: J = (0 + sgn dir, 0 + sgn (x - c_o) x dir) with
// sgn +1 for body a and -1 for body b, Y = (J_lin (1 / m), I_w^-1 J_ang); an absent slot is zero. Used by the families
// that recompute instead of storing them (PhysCfg RC), so every value equals the stored-row value bit for bit.
HD void obj_block(const SimCtx& c, int o, int a, f3 x, f3 dir, float* j6, float* y6) {
    if (o < 0) {
#pragma unroll
        for (int t = 0; t < 6; t++) { j6[t] = 0.0f; y6[t] = 0.0f; }
        return;
    }
    float sgn = o == a ? 1.0f : -1.0f;
    f3 ang = cross3(x - ld3(c.o[o].oc), dir);
    j6[0] = 0.0f + sgn * dir.x; j6[1] = 0.0f + sgn * dir.y; j6[2] = 0.0f + sgn * dir.z;
    j6[3] = 0.0f + sgn * ang.x; j6[4] = 0.0f + sgn * ang.y; j6[5] = 0.0f + sgn * ang.z;
    float im = c.o[o].oc[3];
    y6[0] = j6[0] * im; y6[1] = j6[1] * im; y6[2] = j6[2] * im;
    f3 ya = mv3(c.o[o].oIinv, mk3(j6[3], j6[4], j6[5]));
    y6[3] = ya.x; y6[4] = ya.y; y6[5] = ya.z;
}
// entry t (0..5) of slot object o's block of row direction dir: (J, Y), the values obj_block gives
HD void obj_entry(const SimCtx& c, int o, int a, f3 x, f3 dir, int t, float& j, float& y) {
    float sgn = o == a ? 1.0f : -1.0f;
    f3 ang = cross3(x - ld3(c.o[o].oc), dir);
    f3 jl = mk3(0.0f + sgn * dir.x, 0.0f + sgn * dir.y, 0.0f + sgn * dir.z);
    f3 ja = mk3(0.0f + sgn * ang.x, 0.0f + sgn * ang.y, 0.0f + sgn * ang.z);
    f3 ya = mv3(c.o[o].oIinv, ja);
    float im = c.o[o].oc[3];
    float jv = t == 0 ? jl.x : (t == 1 ? jl.y : (t == 2 ? jl.z : (t == 3 ? ja.x : (t == 4 ? ja.y : ja.z))));
    j = jv;
    y = t < 3 ? jv * im : (t == 3 ? ya.x : (t == 4 ? ya.y : ya.z));
}


// SETS3: the PGS contact loop with its row entries in three register sets that rotate by name (below); a kernel that
// would pay for them in scratch passes false and keeps the copy loop
// YBATCH: the rows phase reads Y_r back in one batch for the diagonal term (below); a kernel that would pay for the
// second register array in scratch, or runs slower with it, passes false and keeps the reload of J_r[i] inside the loop
// (Family rows_y_batch)
template <class PC, bool SETS3 = true, bool YBATCH = true>
HD void substep(SimCtx& c, float hdt) {
    constexpr int ND = PC::nd, NCH = PC::nch, VW = PC::vw;
    constexpr int RSN = row_stride<ND>();
    // the lane id goes through an opaque move each substep: the per-lane 64-bit model addresses are then
    // recomputed here (one or two VALU ops) instead of being hoisted out of the substep loop and spilled
    asm volatile("" : "+v"(c.lane));
    PROF_BEGIN();
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    const ha_params_t& p = *c.p;
    int lane = c.lane, D = c.D, NO = c.NO;
    int NV = D + 6 * NO;
#ifdef HA_AB_DYN_TWICE
    for (int rep = 0; rep < 2; rep++) {
        fk(c);
        dynamics(c);
    }
#else
    fk(c);
    PROF(0);
    dynamics(c);
#endif
    PROF(1);
#ifdef HA_AB_FACTOR_TWICE
    for (int rep = 0; rep < 2; rep++)
#endif
    factor_inverse<ND>(c);
    // free motion: velocity-product forces only (drives are constraint rows of the PGS below)
    if (lane < D) {
        float acc = 0.0f;
        for (int j = 0; j < D; j++) acc = fmaf(c.Minv[lane * D + j], -hdt * s.Cb[j], acc);
        s.v[lane] = s.qd[lane] + acc;
    }
    if (lane < NO) {
        int o = lane;
        float damp = 1.0f / (1.0f + hdt * p.object_ang_damping);
        float R[9], Iw[9], Ii[9], Il[9];
        const float* I0 = m.pool_inertia[c.o[o].pool];
        float sc = c.dr ? c.dr[HA_DR_OBJ_MASS + o] : 1.0f;
        float mass = m.pool_mass[c.o[o].pool];
#pragma unroll
        for (int k = 0; k < 9; k++) Il[k] = I0[k];
        if (body_scaled(c, o)) {
            // uniform density scaled by S: C = tr(I)/2 Id - I (second moments), C' = det(S) S C S,
            // I' = tr(C') Id - C', m' = det(S) m
            const float* sv = c.o[o].osc;
            float det = (sv[0] * sv[1]) * sv[2];
            float h = 0.5f * ((I0[0] + I0[4]) + I0[8]);
            float Cs[9];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) Cs[3 * i + j] = det * (sv[i] * (((i == j ? h : 0.0f) - I0[3 * i + j]) * sv[j]));
            float tr = (Cs[0] + Cs[4]) + Cs[8];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) Il[3 * i + j] = (i == j ? tr : 0.0f) - Cs[3 * i + j];
            mass = mass * det;
        }
        qmat(ldq(c.o[o].oq), R);
        rart3(R, Il, Iw);
#pragma unroll
        for (int k = 0; k < 9; k++) Iw[k] = Iw[k] * sc;
        inv3(Iw, Ii);
#pragma unroll
        for (int k = 0; k < 9; k++) c.o[o].oIinv[k] = Ii[k];
        mass = mass * sc;
        c.o[o].om = mass;
        c.o[o].oc[3] = 1.0f / mass;     // the rows' 1 / m (obj_blocks reads it instead of dividing per PGS fetch)
        // external force and torque (zero unless a task applied them): constant over the call's substeps. Gravity: the
        // shard's randomized sim_params gravity when DR is on (v16)
        const float* grav = c.drg ? c.drg + HA_DRG_GRAVITY : p.gravity;
        f3 lv = (ld3(c.o[o].ov) + ld3(grav) * hdt) + ld3(c.o[o].ofx) * (hdt / mass);
        f3 av = ld3(c.o[o].ow) * damp + mv3(Ii, ld3(c.o[o].otq)) * hdt;
        float* vo = s.v + D + 6 * o;
        vo[0] = lv.x; vo[1] = lv.y; vo[2] = lv.z; vo[3] = av.x; vo[4] = av.y; vo[5] = av.z;
    }
    wsync();
    PROF(2);
#ifdef HA_AB_DETECT_TWICE
    for (int rep = 0; rep < 2; rep++) {
        int nc0 = s.nc;
        wsync();
        c.dry = rep == 1;
        detect<PC::selfc>(c);
        c.dry = false;
        if (rep == 1 && lane == 0) s.nc = nc0;
        wsync();
    }
#else
    detect<PC::selfc>(c);
#endif
    PROF(3);
#ifdef HA_PROFILE
    c.pcls = s.noff > HA_PROFILE_HEAVY ? 1 : 0;
#endif
    if (lane == 0) {        // contact-list diagnostics (ha_state_t.contact_stats)
        int off = s.noff;
        s.cst[0] += 1;
        s.cst[1] += off > c.maxc ? 1 : 0;
        s.cst[2] = off > s.cst[2] ? off : s.cst[2];
        s.cst[3] += off;
    }
    PROF_COUNT(8, s.nc);
    PROF_COUNT(9, 1);
    // ---- contact rows: in chunk ch, lane r < RPC owns global row RPC ch + r (normal, friction 1, friction 2 of
    //      contact CAP ch + r / 3). Rows are packed with the task's stride (J then Y), so a one-object task needs less
    //      LDS (row_stride, task_lds_bytes)
    constexpr int CAP = PC::cap, RPC = PC::rpc;
    float* Jb = s.u.rows.J;
    float* Yb = Jb + RPC * PC::lch * RSN;
    int nc = __builtin_amdgcn_readfirstlane(s.nc);      // wave-uniform (an SGPR: the chunk loops branch on it)
    int nr = 3 * nc;    // nc <= CAP x NCH -> <= RPC x NCH rows
    // split rows (PhysCfg): object blocks of every row (OW wide, J then Y), then the robot blocks of the
    // first KL link contacts (J then Y), then the env's global spill area for the link contacts after those
    constexpr int OW = PC::ow, KL = PC::kl, LCH = PC::lch, SPJ = 3 * (CAP * NCH - KL) * ND;
    float* Ob = Jb;
    float* ObY = Ob + RPC * LCH * OW;
    float* Rb = ObY + RPC * LCH * OW;
    float* RbY = Rb + 3 * KL * ND;
    // overflow chunks (PhysCfg OVF): dense rows of chunks 1.. in the env's global area (J, then Y)
    float* gJ = PC::ovf ? c.spill + PC::off_dense : nullptr;
    float* gY = PC::ovf ? gJ + RPC * (NCH - 1) * RSN : nullptr;
    // contacts that touch a robot link (split rows only): contacts 0..63 in lmask0, 64.. in lmask1
    uint64_t lmask0 = 0, lmask1 = 0;
    if constexpr (PC::split) {
        int a0 = 0, b0 = 0, a1 = 0, b1 = 0;
        if (lane < nc) ct_ab(c, lane, a0, b0);
        lmask0 = __ballot(lane < nc && (a0 >= 100 || b0 >= 100));
        if constexpr (CAP * NCH > 64) {
            if (lane + 64 < nc) ct_ab(c, lane + 64, a1, b1);
            lmask1 = __ballot(lane + 64 < nc && (a1 >= 100 || b1 >= 100));
        }
    }
    // robot-block slot of contact ci (-1: no link), and row k of its J or Y robot block
    auto lslot = [&](int ci) -> int {
        if (CAP * NCH <= 64 || ci < 64)
            return ((lmask0 >> ci) & 1ull) ? (int)__popcll(lmask0 & ((1ull << ci) - 1ull)) : -1;
        int cj = ci - 64;
        return ((lmask1 >> cj) & 1ull) ? (int)(__popcll(lmask0) + __popcll(lmask1 & ((1ull << cj) - 1ull))) : -1;
    };
    auto rrow = [&](int ls, int k, bool y) -> float* {
        if (ls < KL) return (y ? RbY : Rb) + (3 * ls + k) * ND;
        return c.spill + (y ? SPJ : 0) + (3 * (ls - KL) + k) * ND;
    };
    // object blocks (J or Y) of row r in the env's global row area (chunks LCH..)
    auto orow_g = [&](int r, bool y) -> float* {
        return c.spill + PC::spill_robot + (y ? RPC * (NCH - LCH) * OW : 0) + (r - RPC * LCH) * OW;
    };
    // PGS row constants of the lane's row in the current chunk: impulse, target velocity, 1/diagonal, friction and
    // the block's Delassus entries. One chunk: kept in registers. Several: stored per row in RK (after the rows, or
    // for overflow chunks in the env's global area) and swapped into registers chunk by chunk, so registers do not
    // grow with the contact capacity. Overflow chunks: while a substep has <= CAP contacts (chunk 0 only) the
    // constants stay in registers and RK is not touched
    float klam = 0.f, kvt = 0.f, kwinv = 0.f, kcmu = 0.f, kca0 = 0.f, kca1 = 0.f;
    float* RK;
    if constexpr (PC::ovf) RK = c.spill + PC::off_rk;
    else RK = reinterpret_cast<float*>(reinterpret_cast<char*>(s.u.rows.J) + pc_rowdata_bytes<PC>());
    static_assert(PC::rk_stride == RPC * NCH, "RK: one row-constant array per field, every chunk's rows");
    auto rk = [&](int q, int row) -> float& { return RK[q * PC::rk_stride + row]; };   // q < 6, row < rk_stride
    const bool multi = NCH > 1 && (!PC::ovf || nc > CAP);       // wave-uniform
    // packed sweeps (PhysCfg PACK): every substep of the clutter family, the overflow families' substeps whose contacts
    // fit chunk 0. Their row constants go to PK (per contact) instead of registers / RK
    const bool packed = PC::pack && (!PC::ovf || nc <= CAP);           // wave-uniform
    float* PK = PC::pack ? reinterpret_cast<float*>(reinterpret_cast<char*>(s.u.rows.J) + pc_pk_offset<PC>()) : nullptr;
    // robot blocks without the link tree in memory: lane = link holds the link's ancestor DOFs (link_dof_masks), a row
    // lane takes the masks of its two bodies across lanes and evaluates the set DOFs in registers
    const uint32_t am = link_dof_masks(c);
    // chunk ch's rows. LDS (true) / global (false) dense rows are separate instantiations, so that no pointer may
    // address both (a flat pointer would make chunk 0's LDS rows flat accesses too)
    auto rows_chunk = [&](int ch, auto lds_tag) {
        constexpr bool LDSROWS = decltype(lds_tag)::value;
        float vt_ = 0.f, winv_ = 0.f, cmu_ = 0.f;
        int r = RPC * ch + lane;
        // the DOF masks of the row's bodies a and b (0: no link). Before the row lanes diverge: the cross-lane read sees
        // active lanes only
        uint32_t ma = 0u, mb = 0u;
        {
            int a_ = -1, b_ = -1;
            if (lane < RPC && r < nr) ct_ab(c, r / 3, a_, b_);
            uint32_t xa = (uint32_t)lane_read_i((int)am, a_ >= 100 ? a_ - 100 : 0);
            uint32_t xb = (uint32_t)lane_read_i((int)am, b_ >= 100 ? b_ - 100 : 0);
            ma = a_ >= 100 ? xa : 0u;
            mb = b_ >= 100 ? xb : 0u;
        }
        if (lane < RPC && r < nr) {
            const ContactLDS ct = ct_get(c, r / 3);
            cmu_ = contact_friction(c, ct.a, ct.b);
            int k = r % 3;
            // robot block Jr / Yr (null: the contact touches no link, the block is zero) and object blocks Jo / Yo
            float *Jr, *Yr, *Jo, *Yo;
            float jo_rc[PC::rc ? OW : 1], yo_rc[PC::rc ? OW : 1];     // RC: this row's object blocks, in registers
            int ls = -1;                                              // split rows: the contact's link slot
            if constexpr (PC::split) {
                ls = lslot(r / 3);
                Jr = ls >= 0 ? rrow(ls, k, false) : nullptr;
                Yr = ls >= 0 ? rrow(ls, k, true) : nullptr;
                if constexpr (PC::rc) {
                    Jo = jo_rc;
                    Yo = yo_rc;
                } else {
                    if constexpr (LDSROWS) {
                        Jo = Ob + r * OW;
                        Yo = ObY + r * OW;
                    } else {
                        Jo = orow_g(r, false);
                        Yo = orow_g(r, true);
                    }
                    for (int t = 0; t < OW; t++) Jo[t] = 0.0f;
                }
            } else {
                if constexpr (LDSROWS) {
                    Jr = Jb + r * RSN;
                    Yr = Yb + r * RSN;
                } else {
                    Jr = gJ + (r - RPC) * RSN;
                    Yr = gY + (r - RPC) * RSN;
                }
                Jo = Jr + D;
                Yo = Yr + D;
                for (int t = 0; t < RSN - ND; t++) Jo[t] = 0.0f;    // the robot block is stored whole below (D = ND)
            }
            f3 n = ld3(ct.n), t1, t2;
            tangents(n, t1, t2);
            f3 dir = k == 0 ? n : (k == 1 ? t1 : t2);
            f3 x = ld3(ct.x);
            int so0, so1;
            contact_slots(ct.a, ct.b, so0, so1);
            // robot block: entry d is 0, + the a-term if d moves body a, then + the b-term if it moves body b (the sums
            // of oracle/physics_oracle.c:jac_body in its order), summed in a register and stored once. LDS slots / rows
            // and global rows keep their own store paths (no pointer that may address both)
            const bool rl = PC::split ? ls < KL : LDSROWS;      // the robot block is in LDS (else: a global row)
            HA_AS_LDS float *JrL, *YrL;                         // only the pair that rl selects is dereferenced
            HA_AS_GLB float *JrG, *YrG;
            if constexpr (PC::split) {
                JrL = (HA_AS_LDS float*)(Rb + (3 * ls + k) * ND);
                YrL = (HA_AS_LDS float*)(RbY + (3 * ls + k) * ND);
                JrG = (HA_AS_GLB float*)(c.spill + (3 * (ls - KL) + k) * ND);
                YrG = JrG + SPJ;
            } else {
                JrL = (HA_AS_LDS float*)Jr; YrL = (HA_AS_LDS float*)Yr;
                JrG = (HA_AS_GLB float*)Jr; YrG = (HA_AS_GLB float*)Yr;
            }
            if (Jr) {
                // (a rolled loop: unrolled, its 6 x ND LDS loads are scheduled together and spill)
#pragma unroll 1
                for (int d = 0; d < ND; d++) {
                    float v = 0.0f;
                    if (((ma | mb) >> d) & 1u) {
                        float t = dot3(ld3(s.ax[d]), cross3(x - ld3(s.an[d]), dir));
                        if ((ma >> d) & 1u) v += 1.0f * t;
                        if ((mb >> d) & 1u) v += -1.0f * t;
                    }
                    if (rl) JrL[d] = v;
                    else JrG[d] = v;
                }
            }
            if constexpr (PC::rc) {
                // both object blocks (and their Y) straight into registers
                obj_block(c, so0, ct.a, x, dir, jo_rc, yo_rc);
                obj_block(c, so1, ct.a, x, dir, jo_rc + 6, yo_rc + 6);
            } else {
                jac_obj(c, ct.a, x, dir, 1.0f, Jo, so0);
                jac_obj(c, ct.b, x, dir, -1.0f, Jo, so0);
            }
            if (k == 0) {
                float sp = ct.sep;
                float sb = sp + p.contact_slop < 0.0f ? sp + p.contact_slop : 0.0f;   // penetration beyond the slop
                float v0 = sp > 0 ? -sp / hdt : -p.baumgarte * sb / hdt;
                if (v0 > p.max_depen_vel) v0 = p.max_depen_vel;
                vt_ = v0;
            }
            // Y_r = M^-1 J_r^T (robot block through the explicit inverse, object blocks 1/m, I_w^-1). The robot terms of
            // J_r . Y_r (the dense row's first terms, in its order) accumulate here, so Y_r is not read back. An LDS slot /
            // row and a global (spill / overflow) row keep their own typed accesses
            float a = 0.0f;
            if (Jr) {
                // (read back, not kept from the loop over d above: written at a running index the array would live in
                // scratch)
                float jr[ND];
                if (rl) {
#pragma unroll
                    for (int j = 0; j < ND; j++) jr[j] = JrL[j];
                } else {
#pragma unroll
                    for (int j = 0; j < ND; j++) jr[j] = JrG[j];
                }
                constexpr bool YB = YBATCH;
                // the rolled loop stores Y_r[i]. YB: nothing else, and the diagonal terms follow as one chain (i ascending,
                // the dense row's order) over jr and Y_r read back in one batch, both statically indexed, in registers
                // (D = ND): one round trip per row. Otherwise J_r[i] comes from the row again behind each store (the
                // same value), one round trip per DOF
                for (int i = 0; i < D; i++) {
                    float acc = 0.0f;
                    // row i of M^-1 in one batch ahead of the chain (the fence keeps the loads together): left alone the
                    // compiler loads it four entries at a time with a full LDS wait after each load, six round trips per
                    // DOF
                    float mr[ND];
#pragma unroll
                    for (int j = 0; j < ND; j++) mr[j] = c.Minv[i * D + j];
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int j = 0; j < ND; j++) acc = fmaf(mr[j], jr[j], acc);
                    if constexpr (YB) {
                        if (rl) YrL[i] = acc;
                        else YrG[i] = acc;
                    } else {
                        float ji;
                        if (rl) {
                            YrL[i] = acc;
                            ji = JrL[i];
                        } else {
                            YrG[i] = acc;
                            ji = JrG[i];
                        }
                        a = fmaf(ji, acc, a);
                    }
                }
                if constexpr (YB) {
                    float yr[ND];
                    if (rl) {
#pragma unroll
                        for (int i = 0; i < ND; i++) yr[i] = YrL[i];
                    } else {
#pragma unroll
                        for (int i = 0; i < ND; i++) yr[i] = YrG[i];
                    }
#pragma unroll
                    for (int i = 0; i < ND; i++) a = fmaf(jr[i], yr[i], a);
                }
            }
            for (int sl = 0; sl < (PC::rc ? 0 : row_slots<ND>()); sl++) {    // RC: Y already from obj_block
                int o = sl == 0 ? so0 : so1;
                const float* Jos = Jo + 6 * sl;
                float* Yos = Yo + 6 * sl;
                if (o < 0) {
                    for (int t = 0; t < 6; t++) Yos[t] = 0.0f;
                    continue;
                }
                float im = 1.0f / c.o[o].om;
                Yos[0] = Jos[0] * im; Yos[1] = Jos[1] * im; Yos[2] = Jos[2] * im;
                f3 a = mv3(c.o[o].oIinv, mk3(Jos[3], Jos[4], Jos[5]));
                Yos[3] = a.x; Yos[4] = a.y; Yos[5] = a.z;
            }
            // same term order as the dense row: robot block (above), then the object blocks
            for (int t = 0; t < RSN - D; t++) a = fmaf(Jo[t], Yo[t], a);
            winv_ = 1.0f / (a + 1e-9f);
        }
        if (NCH == 1 || (PC::ovf && ch == 0)) {
            kvt = vt_; kwinv = winv_; kcmu = cmu_;
        }
        if (packed) {
            if (lane < RPC && r < nr) {
                int ck = r / 3, k = r - 3 * ck;
                HA_AS_LDS float* q = (HA_AS_LDS float*)(PK + HA_PK * ck);
                q[k] = 0.0f;                                // the impulse
                q[4 + k] = winv_;
                if (k == 0) q[3] = vt_;
                if (k == 1) q[7] = cmu_;
                if (k == 2) q[11] = 0.0f;
            }
        } else if (multi && lane < RPC) {
            rk(0, r) = 0.0f; rk(1, r) = vt_; rk(2, r) = winv_; rk(3, r) = cmu_;
        }
    };
#ifdef HA_AB_ROWS_TWICE     /* A/B timing builds only: the rows phase (rows, then Delassus entries) run twice */
    for (int rep = 0; rep < 2; rep++)
#endif
#pragma unroll 1
    for (int ch = 0; ch < NCH; ch++) {
        if (NCH > 1 && RPC * ch >= nr && (PC::ovf || ch > 0)) break;      // wave-uniform: no rows left
        if (ch < LCH) rows_chunk(ch, std::true_type{});       // LDS rows (every chunk of a dense one-layout family)
        else rows_chunk(ch, std::false_type{});
    }
    wsync();
    // coupling inside each contact's 3-row block (Delassus entries J_ri . M^-1 J_rj^T, i > j): lane of
    // friction row 1 holds a10, lane of friction row 2 holds a20 and a21
    auto delassus_chunk = [&](int ch, auto lds_tag) {
        constexpr bool LDSROWS = decltype(lds_tag)::value;
        float ca0_ = 0.f, ca1_ = 0.f;
        int r = RPC * ch + lane;
        if (lane < RPC && r < nr && r % 3 != 0) {
            int k = r % 3, r0 = r - k;
            const float *Jo, *Y0o;
            float a = 0.0f, b = 0.0f;           // robot-block partial sums (J_rk . Y_r0, J_rk . Y_r1), t = 0 .. D-1
            // one block's terms of both sums: J is loaded once, and the loads of J, Y0 (and for friction row 2, Y1) are
            // issued in batches ahead of the two chains, a over t ascending, then b over t ascending (the rolled loops'
            // order). Statically indexed, in registers; each caller keeps its own address space
            auto bdot = [&](const float* J, const float* Y0, const float* Y1, auto n_tag) {
                constexpr int NT = decltype(n_tag)::value;
                float j[NT], y[NT];
#pragma unroll
                for (int t = 0; t < NT; t++) j[t] = J[t];
#pragma unroll
                for (int t = 0; t < NT; t++) y[t] = Y0[t];
#pragma unroll
                for (int t = 0; t < NT; t++) a = fmaf(j[t], y[t], a);
                if (k == 2) {
#pragma unroll
                    for (int t = 0; t < NT; t++) y[t] = Y1[t];
#pragma unroll
                    for (int t = 0; t < NT; t++) b = fmaf(j[t], y[t], b);
                }
            };
            auto rdot = [&](const float* Jr, const float* Y0r, const float* Y1r) {
                bdot(Jr, Y0r, Y1r, std::integral_constant<int, ND>{});       // D = ND
            };
            float jo_rc[PC::rc ? OW : 1], y0_rc[PC::rc ? 2 * OW : 1];     // RC: J of this row, Y of rows r0, r0 + 1
            if constexpr (PC::split) {
                // LDS slot or global spill row on separate paths, so each keeps its own address space
                int ls = lslot(r / 3);
                if (ls >= 0 && ls < KL) rdot(Rb + (3 * ls + k) * ND, RbY + 3 * ls * ND, RbY + (3 * ls + 1) * ND);
                else if (ls >= KL) {
                    const float* sr = c.spill + 3 * (ls - KL) * ND;
                    rdot(sr + k * ND, sr + SPJ, sr + SPJ + ND);
                }
                if constexpr (PC::rc) {
                    const ContactLDS ct = ct_get(c, r / 3);
                    f3 n = ld3(ct.n), t1, t2;
                    tangents(n, t1, t2);
                    f3 x = ld3(ct.x);
                    int so0, so1;
                    contact_slots(ct.a, ct.b, so0, so1);
                    float scratch[OW];
                    f3 dk = k == 1 ? t1 : t2;
                    obj_block(c, so0, ct.a, x, dk, jo_rc, scratch);
                    obj_block(c, so1, ct.a, x, dk, jo_rc + 6, scratch + 6);
                    obj_block(c, so0, ct.a, x, n, scratch, y0_rc);
                    obj_block(c, so1, ct.a, x, n, scratch + 6, y0_rc + 6);
                    obj_block(c, so0, ct.a, x, t1, scratch, y0_rc + OW);
                    obj_block(c, so1, ct.a, x, t1, scratch + 6, y0_rc + OW + 6);
                    Jo = jo_rc;
                    Y0o = y0_rc;
                } else if constexpr (LDSROWS) {
                    Jo = Ob + r * OW;
                    Y0o = ObY + r0 * OW;
                } else {
                    Jo = orow_g(r, false);
                    Y0o = orow_g(r0, true);
                }
            } else if constexpr (LDSROWS) {
                rdot(Jb + r * RSN, Yb + r0 * RSN, Yb + (r0 + 1) * RSN);
                Jo = Jb + r * RSN + D;
                Y0o = Yb + r0 * RSN + D;
            } else {
                rdot(gJ + (r - RPC) * RSN, gY + (r0 - RPC) * RSN, gY + (r0 + 1 - RPC) * RSN);
                Jo = gJ + (r - RPC) * RSN + D;
                Y0o = gY + (r0 - RPC) * RSN + D;
            }
            const float* Y1o = Y0o + (PC::split ? OW : RSN);
            bdot(Jo, Y0o, Y1o, std::integral_constant<int, RSN - ND>{});
            ca0_ = a;
            if (k == 2) ca1_ = b;
        }
        if (NCH == 1 || (PC::ovf && ch == 0)) {
            kca0 = ca0_; kca1 = ca1_;
        }
        if (packed) {
            if (lane < RPC && r < nr && r % 3 != 0) {
                int ck = r / 3, k = r - 3 * ck;
                HA_AS_LDS float* q = (HA_AS_LDS float*)(PK + HA_PK * ck);
                if (k == 1) q[8] = ca0_;
                else { q[9] = ca0_; q[10] = ca1_; }
            }
        } else if (multi && lane < RPC) {
            rk(4, r) = ca0_; rk(5, r) = ca1_;
        }
    };
#ifdef HA_AB_ROWS_TWICE
    for (int rep = 0; rep < 2; rep++)
#endif
#pragma unroll 1
    for (int ch = 0; ch < NCH; ch++) {
        if (NCH > 1 && RPC * ch >= nr && (PC::ovf || ch > 0)) break;
        if (ch < LCH) delassus_chunk(ch, std::true_type{});
        else delassus_chunk(ch, std::false_type{});
    }
    // ---- free passes (PhysCfg PACK): the contacts that touch no robot link, packed four per pass on pairwise disjoint
    //      objects by a greedy scan in contact order (each pass takes the lowest-index remaining contacts whose objects
    //      the pass does not hold yet: physics_oracle.c packed_passes). A pass is four contact bytes (0xFF: none), in
    //      the union after RK. Lane i holds contacts i and 64 + i; one ballot per pick
    int npass = 0;
    // the pass list stays in registers: pass p is lane p's pair (plo, phi) (p >= 64: plo2, phi2), four 16-bit fields,
    // one per contact: its index (0xFF: none), object slot 0 + 1 and object slot 1 + 1 (contact_slots), so that a
    // sweep decodes a pass from two scalars without an LDS round trip
    uint32_t plo = 0xFFFFFFFFu, phi = 0xFFFFFFFFu, plo2 = 0xFFFFFFFFu, phi2 = 0xFFFFFFFFu;
    if (packed) {
        int o00 = -1, o01 = -1, o10 = -1, o11 = -1;
        if (lane < nc) {
            int a_, b_;
            ct_ab(c, lane, a_, b_);
            o00 = (a_ >= 0 && a_ < 100) ? a_ : -1;
            o01 = (b_ >= 0 && b_ < 100) ? b_ : -1;
        }
        if (CAP * NCH > 64 && lane + 64 < nc) {
            int a_, b_;
            ct_ab(c, lane + 64, a_, b_);
            o10 = (a_ >= 0 && a_ < 100) ? a_ : -1;
            o11 = (b_ >= 0 && b_ < 100) ? b_ : -1;
        }
        uint64_t rem0 = __ballot(lane < nc) & ~lmask0;
        uint64_t rem1 = CAP * NCH > 64 ? __ballot(lane + 64 < nc) & ~lmask1 : 0ull;
        while (rem0 | rem1) {
            uint32_t objm = 0u;
            uint64_t pk = ~0ull;
            uint64_t cand0 = rem0, cand1 = rem1;
            for (int k = 0; k < 4 && (cand0 | cand1); k++) {
                int ci = cand0 ? __ffsll((unsigned long long)cand0) - 1 : 64 + __ffsll((unsigned long long)cand1) - 1;
                int oa = ci < 64 ? __builtin_amdgcn_readlane(o00, ci) : __builtin_amdgcn_readlane(o10, ci - 64);
                int ob = ci < 64 ? __builtin_amdgcn_readlane(o01, ci) : __builtin_amdgcn_readlane(o11, ci - 64);
                objm |= (oa >= 0 ? 1u << oa : 0u) | (ob >= 0 ? 1u << ob : 0u);
                int so0 = oa < 0 ? ob : (ob < 0 ? oa : (oa < ob ? oa : ob));
                int so1 = (oa >= 0 && ob >= 0) ? (oa < ob ? ob : oa) : -1;
                uint64_t fld = (uint64_t)ci | ((uint64_t)(so0 + 1) << 8) | ((uint64_t)(so1 + 1) << 12);
                pk = (pk & ~(0xFFFFull << (16 * k))) | (fld << (16 * k));
                if (ci < 64) rem0 &= ~(1ull << ci);
                else rem1 &= ~(1ull << (ci - 64));
                bool t0 = (o00 >= 0 && ((objm >> o00) & 1u)) || (o01 >= 0 && ((objm >> o01) & 1u));
                bool t1 = (o10 >= 0 && ((objm >> o10) & 1u)) || (o11 >= 0 && ((objm >> o11) & 1u));
                cand0 = rem0 & ~__ballot(t0);
                cand1 = rem1 & ~__ballot(t1);
            }
            if (npass < 64) {
                if (lane == npass) { plo = (uint32_t)pk; phi = (uint32_t)(pk >> 32); }
            } else if (lane == npass - 64) {
                plo2 = (uint32_t)pk; phi2 = (uint32_t)(pk >> 32);
            }
            npass++;
        }
    }
    PROF(4);
    // ---- joint rows, lane d: PD drive (soft implicit spring-damper, |impulse| <= effort h) and the
    //      lower/upper joint limits (hard, unilateral)
    float dgam = 0.f, dbias = 0.f, dwinv = 0.f, dlim = 0.f, dlam = 0.f;
    float lwinv = 0.f, vt_lo = 0.f, vt_up = 0.f, lam_lo = 0.f, lam_up = 0.f;
    // joint friction row (Isaac Gym DOF property "friction", a coefficient: "a generalized friction force is calculated
    // as DOF force multiplied by friction", docs/domain_randomization.md:197): target velocity 0 and
    // |impulse| <= dof_friction |drive + lower - upper impulse| of the DOF, re-bounded each sweep like a contact's
    // friction rows by its normal impulse
    float fcoef = 0.f, lam_fr = 0.f;
    int act_lo = 0, act_up = 0;
    if (lane < D) {
        fcoef = m.dof_friction[lane];
        // DR (v16): the env's dof_properties stiffness / damping / lower / upper (dr_scale row: nominal until sampled)
        float kp = c.dr ? c.dr[HA_DR_DOF_KP + lane] : m.dof_kp[lane];
        float kd = c.dr ? c.dr[HA_DR_DOF_KD + lane] : m.dof_kd[lane];
        float jlo = c.dr ? c.dr[HA_DR_DOF_LOWER + lane] : m.dof_lower[lane];
        float jup = c.dr ? c.dr[HA_DR_DOF_UPPER + lane] : m.dof_upper[lane];
        float den = kd + hdt * kp;
        float mii = c.Minv[lane * D + lane];
        dgam = 1.0f / (hdt * den);
        dbias = kp / den * (s.q[lane] - s.tgt[lane]);
        dwinv = 1.0f / (mii + dgam);
        dlim = m.dof_effort[lane] * hdt;
        lwinv = 1.0f / (mii + 1e-9f);
        float s_lo = s.q[lane] - jlo, s_up = jup - s.q[lane];
        act_lo = s_lo <= p.joint_limit_margin;
        act_up = s_up <= p.joint_limit_margin;
        vt_lo = s_lo > 0 ? -s_lo / hdt : -p.baumgarte * s_lo / hdt;
        vt_up = s_up > 0 ? -s_up / hdt : -p.baumgarte * s_up / hdt;
    }
    const uint64_t lo_mask = __ballot(act_lo != 0), up_mask = __ballot(act_up != 0), fr_mask = __ballot(fcoef > 0.0f);
    // generalized velocity: coordinate `lane` in vreg, coordinate 64 + lane in vregh (VW == 2 only)
    float vreg = lane < NV ? s.v[lane] : 0.0f;
    float vregh = (VW == 2 && lane + 64 < NV) ? s.v[lane + 64] : 0.0f;
    wsync();
    PROF(5);
    // ---- projected Gauss-Seidel (velocity form): joint rows d = 0..D-1 (drive, lower, upper), then
    //      contact rows r = 0..nr-1.  Same row order and arithmetic as the oracle.
    const float* J = Jb;
    const float* Y = Yb;
    // split rows: lane i keeps the link slot of contact i (and of contact 64 + i), -1: no link, so the sweeps read a
    // contact's slot from a register instead of counting mask bits at every fetch
    int lsl0 = -1, lsl1 = -1;
    if constexpr (PC::split && !PC::rc) {
        lsl0 = lslot(lane);
        if (CAP * NCH > 64) lsl1 = lslot(lane + 64);
    }
    // One row slot and split rows (UF below, AllegroKuka): lane i keeps the fetch descriptor of contact i (and of contact
    // 64 + i) instead, one word built here, once per substep, of what a fetch would otherwise derive from the slot per
    // contact and per sweep. Bits 0..13: the byte offset of the contact's object block (12 OW ci: within the LDS object
    // blocks, or from chunk 0's place in the env's global row area when bit 14 is set). Bits 16..29: the byte offset of
    // its robot block (12 ND slot within the LDS slots; 12 ND (slot - KL) within the global spill rows when bit 30 is
    // set; 0 with bit 31 when the contact touches no link)
    constexpr uint32_t FD_OG = 1u << 14, FD_RG = 1u << 30, FD_NL = 1u << 31, FD_GLB = FD_OG | FD_RG;
    auto fdesc = [&](int ci) -> uint32_t {
        int ls = lslot(ci);
        uint32_t fo = 12u * OW * ci | (LCH == NCH || ci < CAP * LCH ? 0u : FD_OG);
        uint32_t fr = ls < 0 ? FD_NL : (ls < KL ? 12u * ND * ls << 16 : (12u * ND * (ls - KL) << 16 | FD_RG));
        return fo | fr;
    };
    // several chunks: the row constants of the chunk after the current one, loaded while the current one is solved
    float sl = 0.f, svt = 0.f, swinv = 0.f, scmu = 0.f, sca0 = 0.f, sca1 = 0.f;
    auto stage = [&](int ch) {
        int row = RPC * ch + lane;
        sl = rk(0, row); svt = rk(1, row); swinv = rk(2, row);
        scmu = rk(3, row); sca0 = rk(4, row); sca1 = rk(5, row);
    };
    if (!packed && multi && lane < RPC) stage(0);
    const int nca = (nc + CAP - 1) / CAP;                   // chunks in use (wave-uniform)
    // the Ur5Sih 3-object family (two row slots, one velocity word): ha_step_kernel sits at its 168 VGPRs with 64
    // B/lane of scratch and the three row sets put it at 72, so it keeps the copy loop
    constexpr bool HA3 = row_slots<ND>() == 2 && VW == 1;
    // joint rows: row d + 1 of S ~ M^-1 is loaded before row d's chain runs (the next sweep's row 0 at d = D - 1), so its
    // LDS latency passes under a whole joint's work. Only the clutter family (two velocity words) has it: its kernel
    // measured 2.9% faster with it, the AllegroHand kernel 1.1% slower, AllegroKuka nothing, and ha_step_kernel pays
    // for the register in scratch (profiles/r08_pgs_sweep.txt)
    constexpr bool JP = VW == 2;
    float mnext = JP && lane < D ? c.Minv[lane] : 0.0f;
    // contact blocks: the row entries of a contact live in one of three register sets that rotate by name. The contact
    // loop is unrolled by three, copy k reads set k and prefetches (two contacts ahead) into the set copy k - 1 has
    // just finished with, so no set is ever copied and the loads go straight into the registers a block reads (the
    // waits the conditional fetch paths still leave: profiles/r08_pgs_sweep.txt, section 4). The copy loop of the
    // other families keeps two sets and rotates the current one by register copies, which wait for the look-ahead loads
    // one block after their issue, and zero-fills the set before every fetch
    struct RowSet {
        float j0 = 0.f, j1 = 0.f, j2 = 0.f, y0 = 0.f, y1 = 0.f, y2 = 0.f;
        float h0 = 0.f, h1 = 0.f, h2 = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;      // coordinate 64 + lane
    };
    // the rotation restarts with every chunk, so a chunk holds whole trips; the two-word family (VW == 2, the clutter
    // kernels at their 168-VGPR cap) would keep 36 row registers in three sets and stays on the copy loop
    constexpr bool ROT = SETS3 && VW == 1 && CAP % 3 == 0 && !HA3;
    // One row slot and split rows (AllegroKuka): a lane's compact index is its own for every contact, so everything
    // per lane in a fetch is fixed here, once per substep: whether it reads an object or a robot block, its offset
    // within the first such block in LDS (from Ob) and in the env's global area (from c.spill), the blocks' row stride
    // and the distance from a J entry to its Y entry. A fetch adds the block offset it cuts out of the contact's
    // descriptor and issues one set of LDS loads in every lane (a lane without an entry reads the zero pad) and, for a
    // contact with a block in the env's global area, one set of global loads in the lanes of that kind
    // (profiles/r09_pgs_fetch.txt). Dense rows with one row slot (AllegroHand) need no zero either: the same lanes load
    // for every contact. The other families zero-fill the set before every fetch, as the copy loop does (it makes
    // every lane wait for the set's previous loads)
    constexpr bool UF = ROT && PC::split && !PC::rc && row_slots<ND>() == 1;
    constexpr bool NZF = UF || (ROT && !PC::split && row_slots<ND>() == 1);
    // (all in bytes, 32 bits: an LDS address is one, and a global load takes the scalar base with a 32-bit lane offset)
    constexpr int oOY = RPC * LCH * OW, oR = 2 * oOY, oRY = oR + 3 * KL * ND;   // ObY, Rb, RbY from Ob, in floats
    const bool f_ob = UF && lane >= D && lane < RSN, f_rb = UF && lane < D;
    // f_sh: where the lane's block offset starts in a contact's descriptor (a lane >= RSN has no block: its LDS loads
    // read the zero pad whatever the field holds, and 0x4000 << 31 is no flag, so it never takes the global set)
    const uint32_t f_sh = f_ob ? 0u : (f_rb ? 16u : 31u);
    const uint32_t f_st = 4u * (f_ob ? OW : ND);
    // LDS addresses (the address space's 32 bits), so that the pad, which lies in front of the rows, is one too
    const uint32_t f_lb = (uint32_t)(uintptr_t)(const HA_AS_LDS float*)Ob;
    const uint32_t f_lo = f_lb + 4u * (f_ob ? lane - D : oR + lane), f_ly = 4u * (f_ob ? oOY : oRY - oR);
    const uint32_t f_go = 4u * (f_ob ? PC::spill_robot - RPC * LCH * OW + (lane - D) : lane);
    const uint32_t f_gy = 4u * (f_ob ? RPC * (NCH - LCH) * OW : SPJ);
    // The zero pad: the last word of the generalized velocity, which no coordinate of this family reaches. A lane
    // without an entry reads it six times (both strides 0): the lanes >= RSN for every contact, the robot lanes for a
    // contact that touches no link. So the LDS set of a fetch runs in every lane, under no lane mask
    const uint32_t f_pad = (uint32_t)(uintptr_t)(const HA_AS_LDS float*)&s.v[MAXV - 1];
    constexpr uint64_t FM_HI = RSN < 64 ? ~0ull << (RSN < 64 ? RSN : 0) : 0ull;                 // lanes >= RSN
    constexpr uint64_t FM_NOB = FM_HI | ((1ull << (ND < 64 ? ND : 0)) - 1ull);                  // ... and the robot lanes
    uint32_t fd0 = 0u, fd1 = 0u;
    if constexpr (UF) {
        static_assert(!UF || ND + 6 * PC::ocap < MAXV, "the zero pad is the velocity's last word");
        static_assert(!UF || (12 * OW * CAP * NCH < (1 << 14) && 12 * ND * CAP * NCH < (1 << 14)), "descriptor fields");
        static_assert(!UF || 12 * OW * CAP * NCH + 4 * (OW + oOY) <= (int)pc_rowdata_bytes<PC>(),
                      "a global object block's offset, read as an LDS one, stays inside the rows");
        fd0 = fdesc(lane);
        if (CAP * NCH > 64) fd1 = fdesc(lane + 64);
        if (lane == 0) *(HA_AS_LDS float*)&s.v[MAXV - 1] = 0.0f;
        wsync();
    }
#ifdef HA_AB_PGS_TWICE
    for (int it = 0; it < 2 * p.solver_iters; it++) {
#else
    for (int it = 0; it < p.solver_iters; it++) {
#endif
        // Each joint row's update is computed by the lane that owns the joint (its own v[d], lambda and row
        // constants: the same operands the oracle uses), and only the impulse change crosses lanes (one
        // v_readlane); the joint-limit rows run only for the joints whose limit is active (ballot masks).
        for (int d = 0; d < D; d++) {
            float mrow;
            if constexpr (JP) {
                mrow = mnext;
                mnext = lane < D ? c.Minv[(d + 1 < D ? d + 1 : 0) * D + lane] : 0.0f;
            } else {
                mrow = lane < D ? c.Minv[d * D + lane] : 0.0f;
            }
            float nl = dlam - (vreg + dbias + dgam * dlam) * dwinv;
            nl = nl < -dlim ? -dlim : (nl > dlim ? dlim : nl);
            float dl = bcast(nl - dlam, d);
            if (dl != 0.0f) {
                if (lane == d) dlam = nl;
                vreg = fmaf(mrow, dl, vreg);
            }
            if ((lo_mask >> d) & 1ull) {
                float n0 = lam_lo - (vreg - vt_lo) * lwinv;
                n0 = n0 < 0.0f ? 0.0f : n0;
                float d0 = bcast(n0 - lam_lo, d);
                if (d0 != 0.0f) {
                    if (lane == d) lam_lo = n0;
                    vreg = fmaf(mrow, d0, vreg);
                }
            }
            if ((up_mask >> d) & 1ull) {
                float n1 = lam_up - (-vreg - vt_up) * lwinv;
                n1 = n1 < 0.0f ? 0.0f : n1;
                float d1 = bcast(n1 - lam_up, d);
                if (d1 != 0.0f) {
                    if (lane == d) lam_up = n1;
                    vreg = fmaf(-mrow, d1, vreg);
                }
            }
            if ((fr_mask >> d) & 1ull) {
                float flim = fcoef * fabsf((dlam + lam_lo) - lam_up);
                float nf = lam_fr - vreg * lwinv;
                nf = nf < -flim ? -flim : (nf > flim ? flim : nf);
                float df = bcast(nf - lam_fr, d);
                if (df != 0.0f) {
                    if (lane == d) lam_fr = nf;
                    vreg = fmaf(mrow, df, vreg);
                }
            }
        }
        // contact blocks: the three J.v reductions of a contact run together; the friction rows see the
        // normal (and first friction) update through the block's Delassus entries, which equals
        // re-reducing J.v after each row (row-by-row Gauss-Seidel) up to rounding
        // lane = generalized coordinate; its entry of a compact row is at compact_index (or absent -> 0).
        // The row entries of the contact two ahead are prefetched while the current one reduces (an overflow chunk's
        // rows and most link contacts' robot blocks come from the env's global area, whose latency one contact of
        // reductions does not cover).
        auto fetch = [&](int ci, RowSet& S) {
            float &j0n = S.j0, &j1n = S.j1, &j2n = S.j2, &y0n = S.y0, &y1n = S.y1, &y2n = S.y2;
            float &h0n = S.h0, &h1n = S.h1, &h2n = S.h2, &g0n = S.g0, &g1n = S.g1, &g2n = S.g2;
            int ix = lane < RSN ? lane : -1;       // one slot: the compact row is the dense row
            int ixh = -1;
            if constexpr (row_slots<ND>() == 2) {
                int ca, cb, so0, so1;
                ct_ab(c, ci, ca, cb);
                contact_slots(ca, cb, so0, so1);
                ix = compact_index(lane, D, so0, so1);
                if (VW == 2) ixh = compact_index(lane + 64, D, so0, so1);
            }
            if constexpr (!NZF) {
                j0n = 0.f; j1n = 0.f; j2n = 0.f; y0n = 0.f; y1n = 0.f; y2n = 0.f;
                h0n = 0.f; h1n = 0.f; h2n = 0.f; g0n = 0.f; g1n = 0.f; g2n = 0.f;
            }
            if constexpr (PC::rc) {
                // object coordinates recomputed from the contact entry (obj_entry: the rows phase's values);
                // robot coordinates from the contact's link slot (LDS for the first KL, else the spill rows)
                const ContactLDS ct = ct_get(c, ci);
                int so0, so1;
                contact_slots(ct.a, ct.b, so0, so1);
                bool o1 = ix >= D, o2 = VW == 2 && ixh >= D;
                if (o1 || o2) {
                    f3 n = ld3(ct.n), t1, t2;
                    tangents(n, t1, t2);
                    f3 x = ld3(ct.x);
                    if (o1) {
                        int t = ix - D, o = t < 6 ? so0 : so1, e = t < 6 ? t : t - 6;
                        obj_entry(c, o, ct.a, x, n, e, j0n, y0n);
                        obj_entry(c, o, ct.a, x, t1, e, j1n, y1n);
                        obj_entry(c, o, ct.a, x, t2, e, j2n, y2n);
                    }
                    if (o2) {
                        int t = ixh - D, o = t < 6 ? so0 : so1, e = t < 6 ? t : t - 6;
                        obj_entry(c, o, ct.a, x, n, e, h0n, g0n);
                        obj_entry(c, o, ct.a, x, t1, e, h1n, g1n);
                        obj_entry(c, o, ct.a, x, t2, e, h2n, g2n);
                    }
                }
                if (ix >= 0 && ix < D) {
                    int ls = lslot(ci);         // wave-uniform: one path per contact, LDS or global
                    if (ls >= 0 && ls < KL) {
                        const float* Rn = Rb + 3 * ls * ND;
                        const float* RYn = RbY + 3 * ls * ND;
                        j0n = Rn[ix]; j1n = Rn[ND + ix]; j2n = Rn[2 * ND + ix];
                        y0n = RYn[ix]; y1n = RYn[ND + ix]; y2n = RYn[2 * ND + ix];
                    } else if (ls >= KL) {
                        const float* Rn = c.spill + 3 * (ls - KL) * ND;
                        const float* RYn = c.spill + SPJ + 3 * (ls - KL) * ND;
                        j0n = Rn[ix]; j1n = Rn[ND + ix]; j2n = Rn[2 * ND + ix];
                        y0n = RYn[ix]; y1n = RYn[ND + ix]; y2n = RYn[2 * ND + ix];
                    }
                }
                return;
            }
            if constexpr (PC::split) {
                // object coordinates from the object blocks (LDS for chunks < LCH, else the env's global row area);
                // robot coordinates from the contact's link slot (LDS for the first KL, else the global spill rows),
                // absent -> 0. LDS and global sources stay on separate paths (both conditions are wave-uniform)
                // the contact's link slot from the lane that holds it (one v_readlane: ci is wave-uniform)
                if constexpr (UF) {
                    // object lanes: the object block of contact ci, in LDS or (chunks LCH..) in the global row area;
                    // robot lanes: the robot block of the contact's slot, in LDS (< KL), in the global spill rows, or
                    // none. All of it comes from the contact's descriptor (one v_readlane: ci is wave-uniform): a lane
                    // cuts its block offset out of the word at its own bit position
                    const uint32_t w = (uint32_t)((CAP * NCH <= 64 || ci < 64) ? bcast_i((int)fd0, ci)
                                                                                : bcast_i((int)fd1, ci - 64));
                    const uint32_t fld = __builtin_amdgcn_ubfe(w, f_sh, 14u);
                    // the LDS set, in every lane and under no lane mask. The lanes without an LDS entry for this contact
                    // read the pad (a scalar mask chosen by the contact's bits): the robot lanes when it touches no link
                    // or its robot block is in the spill rows. (Object lanes whose block is in the global row area read
                    // the LDS object blocks at that offset: inside the rows, and replaced below)
                    {
                        const bool pad = lane_in((w & (FD_NL | FD_RG)) ? FM_NOB : FM_HI);
                        const uint32_t o = pad ? f_pad : f_lo + fld;
                        const uint32_t st = pad ? 0u : f_st, ly = pad ? 0u : f_ly;
                        const uint32_t o1 = o + st, o2 = o1 + st;
                        j0n = *(const HA_AS_LDS float*)(uintptr_t)o;
                        j1n = *(const HA_AS_LDS float*)(uintptr_t)o1;
                        j2n = *(const HA_AS_LDS float*)(uintptr_t)o2;
                        y0n = *(const HA_AS_LDS float*)(uintptr_t)(o + ly);
                        y1n = *(const HA_AS_LDS float*)(uintptr_t)(o1 + ly);
                        y2n = *(const HA_AS_LDS float*)(uintptr_t)(o2 + ly);
                    }
                    // the global set: only for a contact with a global bit (wave-uniform: a scalar branch of its own, which
                    // the empty statement keeps from merging into the lane mask below), in the lanes of that kind
                    if (w & FD_GLB) {
                        asm volatile("");
                        if (w & (0x4000u << f_sh)) {
                            const uint32_t o = f_go + fld;
                            const HA_AS_GLB char* G = (const HA_AS_GLB char*)c.spill;
                            const uint32_t o1 = o + f_st, o2 = o1 + f_st;
                            j0n = *(const HA_AS_GLB float*)(G + o);
                            j1n = *(const HA_AS_GLB float*)(G + o1);
                            j2n = *(const HA_AS_GLB float*)(G + o2);
                            y0n = *(const HA_AS_GLB float*)(G + (o + f_gy));
                            y1n = *(const HA_AS_GLB float*)(G + (o1 + f_gy));
                            y2n = *(const HA_AS_GLB float*)(G + (o2 + f_gy));
                        }
                    }
                    return;
                }
                int lsc = (CAP * NCH <= 64 || ci < 64) ? bcast_i(lsl0, ci) : bcast_i(lsl1, ci - 64);
                bool lds_obj = LCH == NCH || ci < CAP * LCH;
                if (lds_obj && lsc < KL) {
                    // every entry of this contact is in LDS: one set of six LDS loads from one base (the rows' J), each
                    // lane's block (object block of contact ci at stride OW, or robot block of slot lsc at stride ND)
                    // chosen by offsets. The block's offset (3 OW ci | 3 ND lsc) is wave-uniform, scalar arithmetic;
                    // a lane takes one of the two and adds its own offset within the block, which with one object slot
                    // (ix is the lane's own) is invariant over the contacts and the sweeps
                    bool ob = ix >= D, rb = ix >= 0 && ix < D && lsc >= 0;
                    int o0 = ob ? ix - D : oR + ix;
                    int st = ob ? OW : ND;
                    int dy = ob ? oOY : oRY - oR;
                    if (ob || rb) {
                        const int bo = 3 * OW * ci, br = 3 * ND * lsc;      // wave-uniform
                        const HA_AS_LDS float* P = (const HA_AS_LDS float*)Ob + (o0 + (ob ? bo : br));
                        j0n = P[0]; j1n = P[st]; j2n = P[2 * st];
                        y0n = P[dy]; y1n = P[dy + st]; y2n = P[dy + 2 * st];
                    }
                } else if (ix >= D) {
                    int t = ix - D;
                    auto ldo = [&](auto On, auto OYn) {
                        j0n = On[t]; j1n = On[OW + t]; j2n = On[2 * OW + t];
                        y0n = OYn[t]; y1n = OYn[OW + t]; y2n = OYn[2 * OW + t];
                    };
                    if (lds_obj) ldo(lds_f(Ob + 3 * ci * OW), lds_f(ObY + 3 * ci * OW));
                    else ldo(glb_f(orow_g(3 * ci, false)), glb_f(orow_g(3 * ci, true)));
                } else if (ix >= 0) {
                    int ls = lsc;
                    auto ld6 = [&](auto Rn, auto RYn) {
                        j0n = Rn[ix]; j1n = Rn[ND + ix]; j2n = Rn[2 * ND + ix];
                        y0n = RYn[ix]; y1n = RYn[ND + ix]; y2n = RYn[2 * ND + ix];
                    };
                    if (ls >= 0 && ls < KL) ld6(lds_f(Rb + 3 * ls * ND), lds_f(RbY + 3 * ls * ND));
                    else if (ls >= KL) ld6(glb_f(c.spill + 3 * (ls - KL) * ND), glb_f(c.spill + SPJ + 3 * (ls - KL) * ND));
                }
                if (VW == 2 && ixh >= D) {
                    int t = ixh - D;
                    auto ldh = [&](auto On, auto OYn) {
                        h0n = On[t]; h1n = On[OW + t]; h2n = On[2 * OW + t];
                        g0n = OYn[t]; g1n = OYn[OW + t]; g2n = OYn[2 * OW + t];
                    };
                    if (lds_obj) ldh(lds_f(Ob + 3 * ci * OW), lds_f(ObY + 3 * ci * OW));
                    else ldh(glb_f(orow_g(3 * ci, false)), glb_f(orow_g(3 * ci, true)));
                }
                return;
            }
            auto ldd = [&](auto Jn, auto Yn) {
                if (ix >= 0) {
                    j0n = Jn[ix]; j1n = Jn[RSN + ix]; j2n = Jn[2 * RSN + ix];
                    y0n = Yn[ix]; y1n = Yn[RSN + ix]; y2n = Yn[2 * RSN + ix];
                }
                if (VW == 2) {
                    if (ixh >= 0) {
                        h0n = Jn[ixh]; h1n = Jn[RSN + ixh]; h2n = Jn[2 * RSN + ixh];
                        g0n = Yn[ixh]; g1n = Yn[RSN + ixh]; g2n = Yn[2 * RSN + ixh];
                    }
                }
            };
            if (PC::ovf && ci >= CAP) ldd(glb_f(gJ + 3 * (ci - CAP) * RSN), glb_f(gY + 3 * (ci - CAP) * RSN));   // wave-uniform
            else ldd(lds_f(J + 3 * ci * RSN), lds_f(Y + 3 * ci * RSN));
        };
        // packed families: a contact block's constants (impulses, target velocities, 1/diagonals of its three rows, the
        // friction coefficient, the Delassus entries a10 a20 a21) - from RK (LDS), or with overflow chunks from the
        // registers of the lanes that own its rows in chunk 0 - and the serial block's arithmetic on them (n0, d0,
        // hi, n1 through the Delassus entries, n2), evaluated alike by every lane that calls it
        auto consts = [&](int ci, float* K) {                // three 16-byte LDS loads (a broadcast per row)
            typedef float f4v __attribute__((ext_vector_type(4)));
            const HA_AS_LDS f4v* q = (const HA_AS_LDS f4v*)(PK + HA_PK * ci);
            f4v a = q[0], b = q[1], e = q[2];
            K[0] = a.x; K[1] = a.y; K[2] = a.z; K[3] = a.w;
            K[4] = b.x; K[5] = b.y; K[6] = b.z; K[7] = b.w;
            K[8] = e.x; K[9] = e.y; K[10] = e.z;
        };
        // the friction rows' target velocity is 0: x - 0 is x, so the oracle's (jv1 - vt1) is jv1 here
        auto block = [&](const float* K, float jv0, float jv1, float jv2, float& n0, float& n1, float& n2, float& d0,
                         float& d1, float& d2) {
            n0 = K[0] - (jv0 - K[3]) * K[4];
            n0 = n0 < 0.0f ? 0.0f : (n0 > 3.0e38f ? 3.0e38f : n0);
            d0 = n0 - K[0];
            float hi = K[7] * n0;
            n1 = K[1] - fmaf(K[8], d0, jv1) * K[5];
            n1 = n1 < -hi ? -hi : (n1 > hi ? hi : n1);
            d1 = n1 - K[1];
            n2 = K[2] - fmaf(K[10], d1, fmaf(K[9], d0, jv2)) * K[6];
            n2 = n2 < -hi ? -hi : (n2 > hi ? hi : n2);
            d2 = n2 - K[2];
        };
        auto put_lams = [&](int ci, float n0, float n1, float n2) {
            HA_AS_LDS float* q = (HA_AS_LDS float*)(PK + HA_PK * ci);
            q[0] = n0; q[1] = n1; q[2] = n2;
        };
        HA_AS_LDS float* sv = (HA_AS_LDS float*)s.v;      // the generalized velocity of the passes (LDS accesses)
        if (packed) {
            // link contacts: whole-wave blocks in contact order, as the other families solve every contact
            uint64_t lk0 = lmask0, lk1 = lmask1;
            while (lk0 | lk1) {
                int ci = lk0 ? __ffsll((unsigned long long)lk0) - 1 : 64 + __ffsll((unsigned long long)lk1) - 1;
                if (ci < 64) lk0 &= lk0 - 1ull;
                else lk1 &= lk1 - 1ull;
                // no look-ahead here: straight into the set the block reads (zero-filled: a packed family's compact
                // index changes with the contact)
                RowSet S;
                fetch(ci, S);
                const float j0n = S.j0, j1n = S.j1, j2n = S.j2, y0n = S.y0, y1n = S.y1, y2n = S.y2;
                const float h0n = S.h0, h1n = S.h1, h2n = S.h2, g0n = S.g0, g1n = S.g1, g2n = S.g2;
                float jv0 = j0n * vreg, jv1 = j1n * vreg, jv2 = j2n * vreg;
                if (VW == 2) {
                    jv0 = jv0 + h0n * vregh;
                    jv1 = jv1 + h1n * vregh;
                    jv2 = jv2 + h2n * vregh;
                }
                wave_sum_rows3(jv0, jv1, jv2);
                float K[11], n0, n1, n2, d0, d1, d2;
                consts(ci, K);
                block(K, jv0, jv1, jv2, n0, n1, n2, d0, d1, d2);
                if (lane == 0) put_lams(ci, n0, n1, n2);
                if (d0 != 0.0f) { vreg = fmaf(y0n, d0, vreg); if (VW == 2) vregh = fmaf(g0n, d0, vregh); }
                if (d1 != 0.0f) { vreg = fmaf(y1n, d1, vreg); if (VW == 2) vregh = fmaf(g1n, d1, vregh); }
                if (d2 != 0.0f) { vreg = fmaf(y2n, d2, vreg); if (VW == 2) vregh = fmaf(g2n, d2, vregh); }
            }
            // free passes: row rr = lane / 16 takes the pass's contact rr, its lane t < 12 the coordinate t of the
            // contact's compact row (object slot t / 6, entry t % 6). The generalized velocity goes through LDS for the
            // passes (contacts of one pass share no object, so their lanes read and write disjoint coordinates)
            if (npass > 0) {
                if (lane < NV) sv[lane] = vreg;
                if (VW == 2 && lane + 64 < NV) sv[lane + 64] = vregh;
                wsync();
                const int rr = lane >> 4, t = lane & 15;
#pragma unroll 1
                for (int pp = 0; pp < npass; pp++) {
                    uint32_t lo, hi;
                    if (CAP * NCH <= 64 || pp < 64) {
                        lo = __builtin_amdgcn_readlane(plo, pp);
                        hi = __builtin_amdgcn_readlane(phi, pp);
                    } else {
                        lo = __builtin_amdgcn_readlane(plo2, pp - 64);
                        hi = __builtin_amdgcn_readlane(phi2, pp - 64);
                    }
                    uint32_t fld = ((rr < 2 ? lo : hi) >> (16 * (rr & 1))) & 0xFFFFu;
                    int ci = (int)(fld & 0xFFu);
                    bool act = ci != 0xFF;
                    int idx = -1;
                    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, y0 = 0.0f, y1 = 0.0f, y2 = 0.0f, vv = 0.0f;
                    if (act && t < 12) {
                        int o = (int)(t < 6 ? (fld >> 8) & 0xFu : fld >> 12) - 1;
                        if (o >= 0) {
                            idx = D + 6 * o + (t < 6 ? t : t - 6);
                            float j0, j1, j2;
                            if constexpr (PC::ovf) {            // chunk 0's object rows, in LDS
                                auto Jl = lds_f(Ob + 3 * ci * OW);
                                auto Yl = lds_f(ObY + 3 * ci * OW);
                                j0 = Jl[t]; j1 = Jl[OW + t]; j2 = Jl[2 * OW + t];
                                y0 = Yl[t]; y1 = Yl[OW + t]; y2 = Yl[2 * OW + t];
                            } else {                            // the env's global row area
                                auto Jg = glb_f(orow_g(3 * ci, false));
                                auto Yg = glb_f(orow_g(3 * ci, true));
                                j0 = Jg[t]; j1 = Jg[OW + t]; j2 = Jg[2 * OW + t];
                                y0 = Yg[t]; y1 = Yg[OW + t]; y2 = Yg[2 * OW + t];
                            }
                            vv = sv[idx];
                            x0 = j0 * vv; x1 = j1 * vv; x2 = j2 * vv;
                        }
                    }
                    row_sum3(x0, x1, x2);
                    if (act) {
                        float K[11], n0, n1, n2, d0, d1, d2;
                        consts(ci, K);
                        block(K, x0, x1, x2, n0, n1, n2, d0, d1, d2);
                        if (idx >= 0) {
                            if (d0 != 0.0f) vv = fmaf(y0, d0, vv);
                            if (d1 != 0.0f) vv = fmaf(y1, d1, vv);
                            if (d2 != 0.0f) vv = fmaf(y2, d2, vv);
                            sv[idx] = vv;
                        }
                        if (t == 0) put_lams(ci, n0, n1, n2);
                    }
                    wsync();
                }
                vreg = lane < NV ? sv[lane] : 0.0f;
                vregh = (VW == 2 && lane + 64 < NV) ? sv[lane + 64] : 0.0f;
                wsync();
            }
        } else {
        // one contact block: the rows of contact ci (chunk ch) from the set S
        auto solve = [&](int ci, int ch, const RowSet& S) {
            int r0 = 3 * (ci - CAP * ch);       // row of this contact within the chunk (= its lane)
            float jv0 = S.j0 * vreg, jv1 = S.j1 * vreg, jv2 = S.j2 * vreg;
            if (VW == 2) {
                jv0 = jv0 + S.h0 * vregh;
                jv1 = jv1 + S.h1 * vregh;
                jv2 = jv2 + S.h2 * vregh;
            }
            wave_sum_rows3(jv0, jv1, jv2);
            // the block's three rows live in lanes r0, r0 + 1, r0 + 2: each lane evaluates its own row with
            // its own lambda and constants (the oracle's operands) and only n0, d0, d1, d2 cross lanes
            float lm = klam;
            float n0 = lm - (jv0 - kvt) * kwinv;
            n0 = n0 < 0.0f ? 0.0f : (n0 > 3.0e38f ? 3.0e38f : n0);
            float d0 = bcast(n0 - lm, r0);
            n0 = bcast(n0, r0);
            float hi = kcmu * n0;
            float n1 = lm - (fmaf(kca0, d0, jv1) - kvt) * kwinv;
            n1 = n1 < -hi ? -hi : (n1 > hi ? hi : n1);
            float d1 = bcast(n1 - lm, r0 + 1);
            float n2 = lm - (fmaf(kca1, d1, fmaf(kca0, d0, jv2)) - kvt) * kwinv;
            n2 = n2 < -hi ? -hi : (n2 > hi ? hi : n2);
            float d2 = bcast(n2 - lm, r0 + 2);
            if (lane == r0) klam = n0;
            if (lane == r0 + 1) klam = n1;
            if (lane == r0 + 2) klam = n2;
            if (d0 != 0.0f) { vreg = fmaf(S.y0, d0, vreg); if (VW == 2) vregh = fmaf(S.g0, d0, vregh); }
            if (d1 != 0.0f) { vreg = fmaf(S.y1, d1, vreg); if (VW == 2) vregh = fmaf(S.g1, d1, vregh); }
            if (d2 != 0.0f) { vreg = fmaf(S.y2, d2, vreg); if (VW == 2) vregh = fmaf(S.g2, d2, vregh); }
            // the velocity update ends here (an empty statement that pins it): moved down to the next block's products
            // it would read S after the fetch that refills S, and S would be copied (and waited for) first
            if constexpr (ROT) asm volatile("" : "+v"(vreg));
        };
        // set A holds the rows of the contact that starts a trip, B the next one's, C the one after that
        RowSet A, B, C;
        if constexpr (ROT) {
            if (nc > 0) fetch(0, A);
            if (nc > 1) fetch(1, B);
        } else {
            if (nc > 0) { fetch(0, C); B = C; }
            if (nc > 1) fetch(1, C);
        }
#pragma unroll 1
        for (int ch = 0; ch < NCH; ch++) {
            int cend = nc < CAP * (ch + 1) ? nc : CAP * (ch + 1);
            if (NCH > 1) {
                if (CAP * ch >= nc) break;
                if (multi && (nca > 1 || it == 0)) {
                    // this chunk's row constants from the staging registers; the next chunk's (or the next
                    // iteration's chunk 0, whose impulses were stored at its end) are loaded now, under this chunk.
                    // One chunk in use (nca == 1): its constants stay in registers after the first iteration
                    klam = sl; kvt = svt; kwinv = swinv; kcmu = scmu; kca0 = sca0; kca1 = sca1;
                    int nx = (ch + 1 < NCH && CAP * (ch + 1) < nc) ? ch + 1 : 0;
                    if (nca > 1 && lane < RPC) stage(nx);
                }
            }
            if constexpr (ROT) {
                // a trip is three contacts; CAP is a multiple of three, so every chunk starts a trip with set A and
                // only the list's last chunk can end on a part of one (cend == nc there: nothing is left to prefetch)
                int ci = CAP * ch;
#pragma unroll 1
                for (; ci + 3 <= cend; ci += 3) {
                    if (ci + 2 < nc) fetch(ci + 2, C);
                    solve(ci, ch, A);
                    if (ci + 3 < nc) fetch(ci + 3, A);
                    solve(ci + 1, ch, B);
                    if (ci + 4 < nc) fetch(ci + 4, B);
                    solve(ci + 2, ch, C);
                }
                if (ci < cend) {
                    solve(ci, ch, A);
                    if (ci + 1 < cend) solve(ci + 1, ch, B);
                }
            } else {
                for (int ci = CAP * ch; ci < cend; ci++) {
                    RowSet S = B;
                    B = C;
                    if (ci + 2 < nc) fetch(ci + 2, C);
                    solve(ci, ch, S);
                }
            }
            if (multi && lane < RPC) rk(0, RPC * ch + lane) = klam;     // swap the impulses out
        }
        }
    }
    // Joint and contact forces: the last substep wins, like the oracle, and nothing reads them before the launch's
    // final substep has run (PostScratch), so only that substep builds them (wave-uniform)
    if (c.last) {
        // impulse of global row RPC ch + lane (xfer sits before RK / PK in the union: no overlap)
        if (packed) {
            for (int r = lane; r < nr; r += 64) s.u.xfer[r] = ((HA_AS_LDS float*)PK)[HA_PK * (r / 3) + r % 3];
        } else if (!multi) {
            if (lane < RPC) s.u.xfer[lane] = klam;
        } else {
#pragma unroll 1
            for (int ch = 0; ch < NCH; ch++)
                if (lane < RPC && CAP * ch < nc) s.u.xfer[RPC * ch + lane] = rk(0, RPC * ch + lane);
        }
        if (lane < D) s.u.pd.dforce[lane] = (((dlam + lam_lo) - lam_up) + lam_fr) / hdt;
    }
    wsync();
    if (lane < NV) s.v[lane] = vreg;
    if (VW == 2 && lane + 64 < NV) s.v[lane + 64] = vregh;
    PROF(6);
    if (c.last) {
        // each contact's force by a lane of its own, in place over the contact's three impulses
        for (int ci = lane; ci < nc; ci += 64) {
            int r0 = 3 * ci;
            const ContactLDS ct = ct_get(c, ci);
            f3 n = ld3(ct.n), t1, t2;
            tangents(n, t1, t2);
            f3 f = (n * s.u.xfer[r0] + t1 * s.u.xfer[r0 + 1]) + t2 * s.u.xfer[r0 + 2];
            f = f * (1.0f / hdt);
            st3(&s.u.xfer[r0], f);
        }
        wsync();
        // lane = body: its sum runs over the contacts in index order, side a (+) before side b (-), from 0: the
        // order in which the oracle adds into the body's row
        f3 acc = mk3(0.f, 0.f, 0.f);
        for (int ci = 0; ci < nc; ci++) {
            int ba, bb;
            ct_ab(c, ci, ba, bb);
            f3 f = ld3(&s.u.xfer[3 * ci]);
            int ia = ba >= 100 ? m.body_robot0 + (ba - 100) : (ba >= 0 ? m.body_object0 + ba : -1);
            int ib = bb >= 100 ? m.body_robot0 + (bb - 100) : (bb >= 0 ? m.body_object0 + bb : -1);
            if (ia == lane) { acc.x += 1.0f * f.x; acc.y += 1.0f * f.y; acc.z += 1.0f * f.z; }
            if (ib == lane) { acc.x += -1.0f * f.x; acc.y += -1.0f * f.y; acc.z += -1.0f * f.z; }
        }
        if (lane < MAXB) st3(s.u.pd.cforce[lane], acc);
    }
    static_assert(MAXB <= 64, "contact forces: a lane per body");
    wsync();
    // ---- integrate
    if (lane < D) {
        float vv = s.v[lane];
        s.qd[lane] = vv;
        s.q[lane] += hdt * vv;
    }
    if (lane < NO) {
        int o = lane;
        const float* vo = s.v + D + 6 * o;
        f3 lv = mk3(vo[0], vo[1], vo[2]), av = mk3(vo[3], vo[4], vo[5]);
        st3(c.o[o].ov, lv);
        st3(c.o[o].ow, av);
        st3(c.o[o].oc, ld3(c.o[o].oc) + lv * hdt);
        qf q = ldq(c.o[o].oq);
        qf dq = qmul(qf{av.x, av.y, av.z, 0.0f}, q);
        stq(c.o[o].oq, qnormalize(qf{q.x + 0.5f * hdt * dq.x, q.y + 0.5f * hdt * dq.y, q.z + 0.5f * hdt * dq.z,
                                   q.w + 0.5f * hdt * dq.w}));
    }
    wsync();
    PROF(7);
}
