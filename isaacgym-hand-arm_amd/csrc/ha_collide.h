// ha_collide.h - contact detection: poses and scaling, contact emission, SAT and hull-hull narrow phase, boxes, broad
// phase, persistent contact manifolds and the self-collision pass. Third part of ha_physics.h, which includes it after
// ha_dynamics.h (not a header of its own).
#pragma once

struct PoseF { f3 p; qf q; };

// Per-env object dimensions (AllegroKuka's cuboid family): the pool hull of object o is scaled by
// diag(osc[o]) in its body frame. Unscaled bodies (links, static geometry, objects without a scale) take
// the unscaled expressions, bit for bit.
HD bool body_scaled(const SimCtx& c, int b) { return b >= 0 && b < c.NO && c.o[b].osc[3] != 0.0f; }
HD f3 scale3(const SimCtx& c, int b, f3 v) {
    if (!body_scaled(c, b)) return v;
    const float* sc = c.o[b].osc;
    return mk3(v.x * sc[0], v.y * sc[1], v.z * sc[2]);
}
HD float scale_radius(const SimCtx& c, int b, float r) {
    if (!body_scaled(c, b)) return r;
    const float* sc = c.o[b].osc;
    return r * fmaxf(fmaxf(sc[0], sc[1]), sc[2]);
}

HD PoseF object_pose(const SimCtx& c, int o) {
    const EnvLDS& s = *c.s;
    qf q = ldq(c.o[o].oq);
    return PoseF{ld3(c.o[o].oc) - qrot(q, scale3(c, o, ld3(c.m->pool_com[c.o[o].pool]))), q};
}
// object o's pool id when o is wave-uniform (narrow phase): in an SGPR, so the model reads it indexes are scalar
HD int upool(const SimCtx& c, int o) { return __builtin_amdgcn_readfirstlane(c.o[o].pool); }
HD PoseF object_pose_u(const SimCtx& c, int o) {
    qf q = ldq(c.o[o].oq);
    return PoseF{ld3(c.o[o].oc) - qrot(q, scale3(c, o, ld3(c.m->pool_com[upool(c, o)]))), q};
}

// face plane k of a hull in world space; for a scaled body (inv_sc = 1 / scale, read once per hull pair by
// the caller) n' = S^-1 n / |S^-1 n|, d' = d / |S^-1 n|
HD void world_plane(const ha_model_t& m, int hull, int k, PoseF P, bool scaled, f3 inv_sc, f3& n, float& d) {
    const float* pl = m.planes[m.hull_plane_start[hull] + k];
    f3 nl = mk3(pl[0], pl[1], pl[2]);
    float dl = pl[3];
    if (scaled) {
        nl = mk3(pl[0] * inv_sc.x, pl[1] * inv_sc.y, pl[2] * inv_sc.z);
        float inv = 1.0f / sqrtf(dot3(nl, nl));
        nl = nl * inv;
        dl = dl * inv;
    }
    n = qrot(P.q, nl);
    d = dl - dot3(n, P.p);
}
HD f3 inv_scale(const SimCtx& c, int b) {
    if (!body_scaled(c, b)) return mk3(1, 1, 1);
    const float* sc = c.o[b].osc;
    return mk3(1.0f / sc[0], 1.0f / sc[1], 1.0f / sc[2]);
}

HD void store_chosen(SimCtx& c, int k, const f3* P, const f3* N, const float* S, const int* CD, int a, int b);
// A manifold point's anchor for its persistent record (v13; the oracle's PCM_*): the feature it came from - a vertex or
// clipped edge point of side A, of side B, or neither (the midpoint of two edges' closest points) - plus PCM_NORMAL_A
// when the normal is carried by side A (the reference face is A's; B for the ground and edge-edge contacts)
#define PCM_FEAT_A 0
#define PCM_FEAT_B 1
#define PCM_FEAT_MID 2
#define PCM_NORMAL_A 4
// the contacts a pair offers to the list (lane 0; contact_stats columns 3 and 4 via EnvLDS noff / cst)
HD void count_offered(SimCtx& c, int k, int a, int b) {
    EnvLDS& s = *c.s;
    if (c.lane == 0) {
        s.noff += k;
        if (a >= 100 && b >= 100) s.cst[4] += k;
    }
}

// append up to 4 reduced contacts (lane 0 does the list bookkeeping, same policy as the oracle). n is the
// lane's normal: one value over the wave for a convex pair; a compound object pair's gathered points keep
// their piece pair's normal, and the area criterion then measures about the deepest point's normal. While
// c.gather is set (a compound pair's piece pairs) the reduced points go to the gather buffer instead.
HD void emit_contacts(SimCtx& c, bool valid, f3 pt, float sep, f3 n, int a, int b, int code) {
    EnvLDS& s = *c.s;
    int lane = c.lane;
#ifdef HA_AB_TIMING
    if (c.dry) return;
#endif
    // the chosen lanes live in scalars, never in an indexed private array (which would go to scratch)
    float v0 = valid ? sep : 3.0e38f;
    int i0 = valid ? lane : 1 << 20;
    wave_argmin(v0, i0);
    if (i0 >= (1 << 20)) return;
    int k = 1, j1 = 0, j2 = 0, j3 = 0;        // chosen lanes of points 1..3 (valid below k)
    f3 p0 = mk3(bcast(pt.x, i0), bcast(pt.y, i0), bcast(pt.z, i0));
    // points 2-4 only among the candidates within manifold_window of the deepest one (ha_params_t v9)
    bool near = valid && sep <= v0 + c.p->manifold_window;
    f3 dd = pt - p0;
    float v1 = near ? dot3(dd, dd) : -1.0f;
    int i1 = lane;
    wave_argmax(v1, i1);
    if (v1 > 1e-12f) {
        j1 = i1;
        k = 2;
        f3 p1 = mk3(bcast(pt.x, i1), bcast(pt.y, i1), bcast(pt.z, i1));
        f3 e = p1 - p0;
        f3 n0 = mk3(bcast(n.x, i0), bcast(n.y, i0), bcast(n.z, i0));
        float sv = dot3(cross3(e, pt - p0), n0);
        float v2 = near ? sv : -3.0e38f;
        int i2 = lane;
        wave_argmax(v2, i2);
        float v3 = near ? sv : 3.0e38f;
        int i3 = lane;
        wave_argmin(v3, i3);
        bool h2 = v2 > 1e-12f, h3 = v3 < -1e-12f;
        j2 = h2 ? i2 : i3;
        j3 = i3;
        k = 2 + (h2 ? 1 : 0) + (h3 ? 1 : 0);
    }
#ifndef HA_EMIT_PARALLEL
#define HA_EMIT_PARALLEL 1
#endif
    // the chosen lanes' ranks: point t of the manifold (the oracle's idx order)
    int t = lane == i0 ? 0 : (k > 1 && lane == j1 ? 1 : (k > 2 && lane == j2 ? 2 : (k > 3 && lane == j3 ? 3 : -1)));
    if (c.pslot >= 0 && !c.gather) {
        // the pair's manifold for its persistent record (ha_params_t v13), staged in the clipping candidates' scratch
        // (free once the narrow phase has emitted; not part of the hull-side cache): point t = x, n, sep, anchor.
        // pcm_commit writes the record after the pair, at one call site instead of one per emit site
        float* q = reinterpret_cast<float*>(c.col.cand) + 8 * (t < 0 ? 0 : t);
        if (t >= 0) {
            q[0] = pt.x; q[1] = pt.y; q[2] = pt.z; q[3] = n.x; q[4] = n.y; q[5] = n.z; q[6] = sep;
            q[7] = __int_as_float(code);
        }
        c.pemit = k;
    }
    if (HA_EMIT_PARALLEL && !c.gather) {
        int nc0 = s.nc;
        if (nc0 + k <= c.maxc) {
            // room for all k points (the common case): each chosen lane writes its own point into slot nc + t,
            // the values lane 0 would write after broadcasting them (the chosen lanes are distinct)
            count_offered(c, k, a, b);
            if (lane == 0) s.nc = nc0 + k;
            if (t >= 0) ct_put(c, nc0 + t, pt, n, sep, a, b);
            wsync();
            return;
        }
    }
    // the chosen points to every lane
    f3 P[4], N[4];
    float S[4];
    int CD[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        int src = t == 0 ? i0 : (t < k ? (t == 1 ? j1 : (t == 2 ? j2 : j3)) : 0);
        P[t] = mk3(bcast(pt.x, src), bcast(pt.y, src), bcast(pt.z, src));
        N[t] = mk3(bcast(n.x, src), bcast(n.y, src), bcast(n.z, src));
        S[t] = bcast(sep, src);
        CD[t] = bcast_i(code, src);
    }
    store_chosen(c, k, P, N, S, CD, a, b);
}

// the k <= 4 chosen points of a manifold (wave-uniform P, N, S) into the gather buffer (a compound pair's piece
// pairs) or the contact list: lane 0 appends, or (list full) replaces the shallowest contact if the new one is deeper
HD void store_chosen(SimCtx& c, int k, const f3* P, const f3* N, const float* S, const int* CD, int a, int b) {
    EnvLDS& s = *c.s;
    int lane = c.lane;
    if (c.gather) {
        // compound pair: the chosen points (in the oracle's index order) join the gather buffer
        if (lane == 0) {
            const ColView& cs = c.col;
            int ng = s.ng;
#pragma unroll
            for (int t = 0; t < 4; t++) {
                if (t < k && ng < HA_MAX_GATHER) {
                    st3(cs.gp[ng], P[t]);
                    cs.gp[ng][3] = S[t];
                    st3(cs.gn[ng], N[t]);
                    cs.gn[ng][3] = __int_as_float(CD[t]);       // the point's persistent-record anchor
                    ng++;
                }
            }
            s.ng = ng;
        }
        wsync();
        return;
    }
    count_offered(c, k, a, b);
    // lane 0 appends, or (list full) replaces the shallowest contact if this one is deeper: the shallowest is the first
    // maximum of sep over the list (the oracle's sequential strict-compare scan), found by a wave arg-max over
    // lanes = contacts instead of a scan on lane 0 (clutter scenes run with the list full)
#pragma unroll
    for (int t = 0; t < 4; t++) {
        if (t >= k) break;
        int nc = s.nc, slot;
        if (nc >= c.maxc) {
            float sv = lane < c.maxc ? ct_sep(c, lane) : -3.0e38f;
            int w = lane;
            if (c.maxc > 64) {          // contacts 64.. in the same lanes; a tie keeps the lower index
                float s2 = lane + 64 < c.maxc ? ct_sep(c, lane + 64) : -3.0e38f;
                if (s2 > sv) { sv = s2; w = lane + 64; }
            }
            wave_argmax(sv, w);
            if (sv <= S[t]) continue;
            slot = w;
        } else {
            slot = nc;
        }
        if (lane == 0) {
            if (slot == nc) s.nc = nc + 1;
            ct_put(c, slot, P[t], N[t], S[t], a, b);
        }
        wsync();
    }
    wsync();
}

HD void collide_ground(SimCtx& c, int hull, PoseF P, int a) {
    const ha_model_t& m = *c.m;
    float mg = c.p->contact_margin;
    f3 ctr = P.p + qrot(P.q, scale3(c, a, ld3(m.hull_center[hull])));
    if (ctr.z - scale_radius(c, a, m.hull_radius[hull]) > mg) return;
    int lane = c.lane;
    bool valid = false;
    f3 pt = mk3(0, 0, 0);
    float sep = 0;
    if (lane < m.hull_nverts[hull]) {
        f3 v = P.p + qrot(P.q, scale3(c, a, ld3(m.verts[m.hull_vert_start[hull] + lane])));
        if (v.z <= mg) {
            valid = true;
            pt = v - mk3(0, 0, 0.5f * v.z);
            sep = v.z;
        }
    }
    emit_contacts(c, valid, pt, sep, mk3(0, 0, 1), a, -1, PCM_FEAT_A);
}

// float <-> int mapping that preserves order (for LDS atomicMax over floats)
HD int f2ord(float f) {
    int i = __float_as_int(f);
    return i >= 0 ? i : i ^ 0x7fffffff;
}
HD float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// SAT over the face planes wp[0..np) of one hull against the world vertices wv[0..nv) of the other:
// sep = max_k min_i (n_k . v_i + d_k), k = its argmax (ties -> smaller k). Every (k, i) value is the
// same expression as in the oracle; only the parallel order of the (exact) min/max differs.
HD void sat_planes(const SimCtx& c, const float (*wp)[4], int np, const float (*wv)[4], int nv, float& sep, int& kbest) {
    int lane = c.lane;
    if (np <= 8) {
        // few planes (boxes): lane = (plane k = lane / 8, vertex group g = lane % 8). A lane takes the min over its
        // group's vertices g, g + 8, ..., then the plane's eight lanes combine (quad_perm xor1, xor2,
        // row_half_mirror: a min inside each 8-lane group), then one wave max over the planes; its first k is the
        // lowest lane holding it (the oracle's strict-compare scan keeps the first maximum). Every (k, i) value is
        // the oracle's expression and min / max are exact, so the order does not matter
        int k = lane >> 3, g = lane & 7;
        float m = 3.0e38f;
        if (k < np) {
            f3 n = ld3(wp[k]);
            float d = wp[k][3];
#pragma unroll 1
            for (int i = g; i < nv; i += 8) m = fminf(m, dot3(n, ld3(wv[i])) + d);
        }
        m = fminf(m, dpp_f<0xB1>(m));
        m = fminf(m, dpp_f<0x4E>(m));
        m = fminf(m, dpp_f<0x141>(m));
        float v = k < np ? m : -3.0e38f;
        float best = wave_max(v);
        uint64_t hit = __ballot(k < np && v == best);
        sep = best;
        kbest = (int)((__ffsll((unsigned long long)hit) - 1) >> 3);
        return;
    }
    // lane = plane (k = lane, lane + 64), loop over the vertices with batched LDS loads
    float best = -3.0e38f;
    int bk = 1 << 20;
    for (int k = lane; k < np; k += 64) {
        f3 n = ld3(wp[k]);
        float d = wp[k][3];
        float m0 = 3.0e38f, m1 = 3.0e38f;
        int i = 0;
        for (; i + 4 <= nv; i += 4) {
            float4 a = *reinterpret_cast<const float4*>(wv[i]);
            float4 b = *reinterpret_cast<const float4*>(wv[i + 1]);
            float4 e = *reinterpret_cast<const float4*>(wv[i + 2]);
            float4 f = *reinterpret_cast<const float4*>(wv[i + 3]);
            m0 = fminf(m0, dot3(n, mk3(a.x, a.y, a.z)) + d);
            m1 = fminf(m1, dot3(n, mk3(b.x, b.y, b.z)) + d);
            m0 = fminf(m0, dot3(n, mk3(e.x, e.y, e.z)) + d);
            m1 = fminf(m1, dot3(n, mk3(f.x, f.y, f.z)) + d);
        }
        for (; i < nv; i++) m0 = fminf(m0, dot3(n, ld3(wv[i])) + d);
        float mn = fminf(m0, m1);
        if (mn > best) { best = mn; bk = k; }
    }
    wave_argmax(best, bk);
    sep = best;
    kbest = bk;
}

// squared distance from point q to the segment p0 + t (p1 - p0), t in [0, 1] (the oracle's seg_point_d2)
HD float seg_point_d2(f3 p0, f3 p1, f3 q) {
    f3 d = p1 - p0;
    float dd = dot3(d, d);
    float t = dd > 0.0f ? dot3(q - p0, d) / dd : 0.0f;
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
    f3 r = q - (p0 + d * t);
    return dot3(r, r);
}
// the edges of one hull (records E[0..ne), world vertices wv) within sqrt(r2) of the other hull's centre ctr, as a
// byte list of edge indices in edge order (an edge farther away cannot touch the other hull); returns the count
HD int edge_cull(const SimCtx& c, const uint32_t* E, int ne, const float (*wv)[4], f3 ctr, float r2, uint8_t* out) {
    int n = 0;
#pragma unroll 1
    for (int base = 0; base < ne; base += 64) {
        int i = base + c.lane;
        bool keep = false;
        if (i < ne) {
            uint32_t e = E[i];
            keep = seg_point_d2(ld3(wv[e & 255u]), ld3(wv[(e >> 8) & 255u]), ctr) <= r2;
        }
        uint64_t mk = __ballot(keep);
        if (keep) out[n + __popcll(mk & ((1ull << c.lane) - 1ull))] = (uint8_t)i;
        n += __popcll(mk);
    }
    return n;
}
// Edge pair (ea of hull A, eb of hull B; edge records v0 | v1 << 8 | f0 << 16 | f1 << 24) of the edge-edge SAT
// (Gregorius, GDC 2013): when the Gauss-map arcs of the two edges (between their faces' normals; B's negated)
// cross, the pair is a face of the Minkowski difference and N = e1 x e2, oriented away from B's centre cb, is a
// separating-axis candidate with separation N . (pA - pB). Returns -3e38 for any other pair (arcs apart, or edges
// within 0.3 degrees of parallel). n, pa / e1, pb / e2: the axis and the edges (start, direction).
HD float edge_axis(const ColView& cs, uint32_t ea, uint32_t eb, f3 cb, f3& n, f3& pa, f3& e1, f3& pb, f3& e2) {
    // the outputs are set on every path (the caller reads them after the winning pair's call)
    pa = ld3(cs.wvA[ea & 255u]);
    e1 = ld3(cs.wvA[(ea >> 8) & 255u]) - pa;
    pb = ld3(cs.wvB[eb & 255u]);
    e2 = ld3(cs.wvB[(eb >> 8) & 255u]) - pb;
    n = cross3(e1, e2);
    f3 a = ld3(cs.wpA[(ea >> 16) & 255u]), b = ld3(cs.wpA[ea >> 24]);
    f3 cc = ld3(cs.wpB[(eb >> 16) & 255u]) * -1.0f, dd = ld3(cs.wpB[eb >> 24]) * -1.0f;
    f3 bxa = cross3(b, a), dxc = cross3(dd, cc);
    float cba = dot3(cc, bxa), dba = dot3(dd, bxa), adc = dot3(a, dxc), bdc = dot3(b, dxc);
    if (!(cba * dba < 0.0f && adc * bdc < 0.0f && cba * bdc > 0.0f)) return -3.0e38f;
    float l2 = dot3(n, n);
    if (l2 < 2.5e-5f * (dot3(e1, e1) * dot3(e2, e2))) return -3.0e38f;
    n = n * (1.0f / sqrtf(l2));
    if (dot3(n, pb - cb) < 0.0f) n = n * -1.0f;
    return dot3(n, pa - pb);
}
// midpoint of the closest points of the segments pa + s e1 and pb + t e2 (s, t in [0, 1]; not parallel)
HD f3 edge_closest_mid(f3 pa, f3 e1, f3 pb, f3 e2) {
    f3 r = pa - pb;
    float aa = dot3(e1, e1), ee = dot3(e2, e2), bb = dot3(e1, e2), cc = dot3(e1, r), ff = dot3(e2, r);
    float den = aa * ee - bb * bb;
    float sa = den > 0.0f ? (bb * ff - cc * ee) / den : 0.0f;
    sa = sa < 0.0f ? 0.0f : (sa > 1.0f ? 1.0f : sa);
    float tb = (bb * sa + ff) / ee;
    if (tb < 0.0f) {
        tb = 0.0f;
        sa = -cc / aa;
        sa = sa < 0.0f ? 0.0f : (sa > 1.0f ? 1.0f : sa);
    } else if (tb > 1.0f) {
        tb = 1.0f;
        sa = (bb - cc) / aa;
        sa = sa < 0.0f ? 0.0f : (sa > 1.0f ? 1.0f : sa);
    }
    return ((pa + e1 * sa) + (pb + e2 * tb)) * 0.5f;
}

// hull A (body a) vs hull B (body b); normal from B to A. keyA / keyB identify the posed hull of each side for
// the ColScratch cache (the body code, or -100 - k for static body k: statics may share a hull)
HD void collide_hulls(SimCtx& c, int ha, PoseF PA, int hb, PoseF PB, int a, int b, int keyA, int keyB) {
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    float mg = c.p->contact_margin;
    int lane = c.lane;
    f3 ca = PA.p + qrot(PA.q, scale3(c, a, ld3(m.hull_center[ha])));
    f3 cb = PB.p + qrot(PB.q, scale3(c, b, ld3(m.hull_center[hb])));
    f3 dc = ca - cb;
    float rr = scale_radius(c, a, m.hull_radius[ha]) + scale_radius(c, b, m.hull_radius[hb]) + mg;
    c.sepf = 0xFF;
    if (dot3(dc, dc) > rr * rr) return;
    int nva = m.hull_nverts[ha], nvb = m.hull_nverts[hb];
    int npa = m.hull_nplanes[ha], npb = m.hull_nplanes[hb];
    const ColView& cs = c.col;
#ifdef HA_PROFILE
    unsigned long long _h0 = __builtin_amdgcn_s_memtime();
#define HPROF(i) do { wsync(); unsigned long long _h1 = __builtin_amdgcn_s_memtime(); PROF_COUNT(i, _h1 - _h0); \
                          PROF_COUNT(32 + 8 * c.pk + (i) - 25, _h1 - _h0); _h0 = _h1; } while (0)
#else
#define HPROF(i)
#endif
    // world vertices and planes of both hulls, unless this side's (hull, body) is already in ColScratch
    bool needA = ha != c.colA_h || keyA != c.colA_b, needB = hb != c.colB_h || keyB != c.colB_b;
    if (needB) {
        if (lane < nvb) st3(cs.wvB[lane], PB.p + qrot(PB.q, scale3(c, b, ld3(m.verts[m.hull_vert_start[hb] + lane]))));
        bool scB = body_scaled(c, b);
        f3 isB = inv_scale(c, b);
        for (int k = lane; k < npb; k += 64) {
            f3 n; float d;
            world_plane(m, hb, k, PB, scB, isB, n, d);
            st3(cs.wpB[k], n);
            cs.wpB[k][3] = d;
        }
        c.colB_h = hb; c.colB_b = keyB;
        wsync();
    }
    // side A's bounding sphere against B's face planes before A's setup: a plane the sphere clears by more than
    // the margin (with a 1 mm allowance for rounding) clears every vertex of A too, so SAT over B's planes would
    // separate the pair; such a pair (most link hulls near an object) skips A's setup and the SAT. No result
    // changes: the oracle runs the full test and finds the same separation
    if (c.p->narrow_phase_flags & HA_NP_NO_SPHERE_CULL) {
    } else {
        float sc = -3.0e38f;
        int kc = 1 << 20;
        for (int k = lane; k < npb; k += 64) {
            float v = dot3(ld3(cs.wpB[k]), ca) + cs.wpB[k][3];
            if (v > sc) { sc = v; kc = k; }
        }
        float scm = wave_max(sc);
        if (scm - scale_radius(c, a, m.hull_radius[ha]) > mg + 1e-3f) {
            if (c.selfc || c.pairf) {       // B's face k separates A: the hint the pair's next detection checks first
                wave_argmax(sc, kc);
                c.sepf = 0x80 | kc;
            }
            return;
        }
    }
    if (needA) {
        if (lane < nva) st3(cs.wvA[lane], PA.p + qrot(PA.q, scale3(c, a, ld3(m.verts[m.hull_vert_start[ha] + lane]))));
        c.colA_h = ha; c.colA_b = keyA; c.colA_p = false;
        wsync();
    }
    HPROF(25);
    // B's face planes against A's vertices first: side A's planes (a link hull's up to 60) are only built when
    // that test does not separate the pair. Either test alone separating means no contact, so the order changes
    // no result
    float sepA, sepB;
    int kA, kB;
    sat_planes(c, cs.wpB, npb, cs.wvA, nva, sepB, kB);
    HPROF(27);
    if (sepB > mg) {
        c.sepf = 0x80 | kB;
        return;
    }
    if (!c.colA_p) {
        bool scA = body_scaled(c, a);
        f3 isA = inv_scale(c, a);
        for (int k = lane; k < npa; k += 64) {
            f3 n; float d;
            world_plane(m, ha, k, PA, scA, isA, n, d);
            st3(cs.wpA[k], n);
            cs.wpA[k][3] = d;
        }
        c.colA_p = true;
        wsync();
    }
    HPROF(25);
    sat_planes(c, cs.wpA, npa, cs.wvB, nvb, sepA, kA);
    HPROF(26);
    if (sepA > mg) {
        c.sepf = kA;
        return;
    }
    // ---- edge-edge axes (v10): a hull pair whose face axes leave it within the margin may still be separated along,
    //      or touch through, a pair of edges
    int nea = m.hull_nedges[ha], neb = m.hull_nedges[hb];
    if (c.p->narrow_phase_flags & HA_NP_NO_EDGE_AXES) nea = 0;
    if (nea > 0 && neb > 0) {
        float smax = fmaxf(sepA, sepB);
        float pen = smax < 0.0f ? -smax : 0.0f;
        float RA = (scale_radius(c, a, m.hull_radius[ha]) + mg) + pen;
        float RB = (scale_radius(c, b, m.hull_radius[hb]) + mg) + pen;
        uint8_t* la = reinterpret_cast<uint8_t*>(cs.cand);
        uint8_t* lb = reinterpret_cast<uint8_t*>(cs.cmax);
        const uint32_t* EA = m.edges + m.hull_edge_start[ha];
        const uint32_t* EB = m.edges + m.hull_edge_start[hb];
        // side B first (the static box, or the object of a link pair): its list is empty for most pairs (a table's
        // edges are far from an object resting on its face), and then no pair exists and side A's cull is skipped
        int nB = edge_cull(c, EB, neb, cs.wvB, ca, RA * RA, lb);
        int nA = nB > 0 ? edge_cull(c, EA, nea, cs.wvA, cb, RB * RB, la) : 0;
        wsync();
        float best = -3.0e38f;
        int bw = 1 << 30;
        // pairs (i, j) of the two lists, w = i nB + j: the lanes take the elements of the longer list (64 at a time)
        // and loop over the shorter one, whose element is wave-uniform per iteration. Per-edge terms (start,
        // direction, face normals, the Gauss-arc normal, the B edge's offset from cb) are formed once per element,
        // by the same expressions edge_axis evaluates per pair; the winner (max, then lowest w) is the oracle's
        // i-major scan
        if (nA > 0 && nB > 0) {
            bool aLong = nA >= nB;
            int nL = aLong ? nA : nB, nS = aLong ? nB : nA;
            const uint8_t* lL = aLong ? la : lb;
            const uint8_t* lS = aLong ? lb : la;
            const uint32_t* EL = aLong ? EA : EB;
            const uint32_t* ES = aLong ? EB : EA;
            const float (*wvL)[4] = aLong ? cs.wvA : cs.wvB;
            const float (*wvS)[4] = aLong ? cs.wvB : cs.wvA;
            const float (*wpL)[4] = aLong ? cs.wpA : cs.wpB;
            const float (*wpS)[4] = aLong ? cs.wpB : cs.wpA;
            // the short list's records, element t in lane t (t < 64)
            uint32_t recS = lane < nS ? ES[lS[lane]] : 0u;
#pragma unroll 1
            for (int base = 0; base < nL; base += 64) {
                int li = base + lane;
                bool act = li < nL;
                uint32_t rl = act ? EL[lL[li]] : EL[lL[0]];
                // this lane's edge: A side (pa, e1, a, b, bxa) or B side (pb, e2, -f0, -f1, dxc, pb - cb)
                f3 lp = ld3(wvL[rl & 255u]);
                f3 le = ld3(wvL[(rl >> 8) & 255u]) - lp;
                f3 lf0 = ld3(wpL[(rl >> 16) & 255u]), lf1 = ld3(wpL[rl >> 24]);
                if (!aLong) { lf0 = lf0 * -1.0f; lf1 = lf1 * -1.0f; }
                f3 lx = cross3(lf1, lf0);
                f3 lo = lp - cb;
                // two passes per 64 short-list edges: (1) the Gauss-map test of this lane's edge against each of them
                // (wave-uniform short edge, its face normals broadcast from LDS) into a bit mask; (2) each lane walks
                // its own passing pairs in increasing order and evaluates their axes. The same pairs, values and
                // first-max-wins order as one loop evaluating every pair, but the axis arithmetic runs only on the
                // lanes whose pair passed instead of on the whole wave whenever any lane's did
#pragma unroll 1
                for (int sb = 0; sb < nS; sb += 64) {
                    int ns = nS - sb < 64 ? nS - sb : 64;
                    uint64_t pm = 0;
#pragma unroll 1
                    for (int t = 0; t < ns; t++) {
                        int si = sb + t;
                        uint32_t rs = si < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)recS, si)
                                              : ES[__builtin_amdgcn_readfirstlane(lS[si])];
                        f3 sf0 = ld3(wpS[(rs >> 16) & 255u]), sf1 = ld3(wpS[rs >> 24]);
                        if (aLong) { sf0 = sf0 * -1.0f; sf1 = sf1 * -1.0f; }
                        f3 sx = cross3(sf1, sf0);
                        // A: (a, b, bxa) = (f0, f1, f1 x f0); B: (c, d, dxc) = (-f0, -f1, (-f1) x (-f0))
                        f3 a = aLong ? lf0 : sf0, b = aLong ? lf1 : sf1, bxa = aLong ? lx : sx;
                        f3 cc = aLong ? sf0 : lf0, dd = aLong ? sf1 : lf1, dxc = aLong ? sx : lx;
                        float cba = dot3(cc, bxa), dba = dot3(dd, bxa), adc = dot3(a, dxc), bdc = dot3(b, dxc);
                        bool pass = cba * dba < 0.0f && adc * bdc < 0.0f && cba * bdc > 0.0f;
                        pm |= (uint64_t)(pass ? 1u : 0u) << t;
                    }
                    if (!act) pm = 0;
#pragma unroll 1
                    while (__ballot(pm != 0) != 0ull) {
                        // (the short edge's record comes from its lane with every lane active: a lane permute whose
                        // source lane is inactive would not read its value)
                        int t = pm != 0 ? __ffsll((unsigned long long)pm) - 1 : 0;
                        int si = sb + t;
                        uint32_t rs = (uint32_t)__shfl((int)recS, t);
                        if (pm == 0) continue;
                        pm &= pm - 1;
                        if (sb > 0) rs = ES[lS[si]];
                        f3 sp = ld3(wvS[rs & 255u]);
                        f3 se = ld3(wvS[(rs >> 8) & 255u]) - sp;
                        f3 pa = aLong ? lp : sp, e1 = aLong ? le : se, pb = aLong ? sp : lp, e2 = aLong ? se : le;
                        f3 n = cross3(e1, e2);
                        float l2 = dot3(n, n);
                        if (l2 < 2.5e-5f * (dot3(e1, e1) * dot3(e2, e2))) continue;
                        n = n * (1.0f / sqrtf(l2));
                        f3 pbo = aLong ? sp - cb : lo;
                        if (dot3(n, pbo) < 0.0f) n = n * -1.0f;
                        float sv = dot3(n, pa - pb);
                        int w = aLong ? li * nB + si : si * nB + li;
                        if (sv > best) { best = sv; bw = w; }
                    }
                }
            }
        }
        if (nA > 0 && nB > 0) wave_argmax(best, bw);      // (no pair: best stays -3e38, no reduction needed)
        HPROF(30);
        if (best > mg) return;                              // separated along an edge-edge axis
        if (best > c.p->edge_rel_tol * smax + c.p->edge_abs_tol) {
            // edge contact: one point midway between the edges' closest points, normal the axis
            int bi = bw / nB;
            f3 n, pa, pb, e1, e2;
            edge_axis(cs, EA[la[bi]], EB[lb[bw - bi * nB]], cb, n, pa, e1, pb, e2);
            f3 x = edge_closest_mid(pa, e1, pb, e2);
            emit_contacts(c, lane == 0, x, best, n, a, b, PCM_FEAT_MID);
            return;
        }
        wsync();                                            // the edge lists (cand / cmax) are reused below
    }
    // ---- face contact: the reference face (the face axis of larger separation; the other if it yields nothing) and
    //      the incident hull, candidates (1) incident vertices near the reference face and inside its hull's other
    //      planes, (2) the incident face's edges clipped to the reference face's side planes, (3) the reference face's
    //      vertices over the incident face
    for (int pass = 0; pass < 2; pass++) {
        bool refB = (sepB >= sepA) ? (pass == 0) : (pass == 1);
        int kr = refB ? kB : kA;
        int hr = refB ? hb : ha, hi = refB ? ha : hb;
        int nvi = refB ? nva : nvb, npr = refB ? npb : npa, npi = refB ? npa : npb;
        const float (*wpr)[4] = refB ? cs.wpB : cs.wpA;
        const float (*wpi)[4] = refB ? cs.wpA : cs.wpB;
        const float (*wvi)[4] = refB ? cs.wvA : cs.wvB;
        const float (*wvr)[4] = refB ? cs.wvB : cs.wvA;
        f3 nref = ld3(wpr[kr]);
        float dref = wpr[kr][3];
        // (1) incident vertices within the margin of the reference face
        f3 vi = mk3(0, 0, 0);
        float dist = 0;
        bool cand = false;
        if (lane < nvi) {
            vi = ld3(wvi[lane]);
            dist = dot3(nref, vi) + dref;
            cand = dist <= mg;
        }
        uint64_t cm = __ballot(cand);
        int ncand = __popcll(cm);
        int slot = __popcll(cm & ((1ull << lane) - 1ull));
        if (cand) {
            cs.cand[slot] = lane;
            cs.cmax[slot] = f2ord(-3.0e38f);
        }
        wsync();
        // side planes of the reference face: max distance per candidate over (candidate, plane) pairs
        // spread across the lanes (exact max -> order-independent)
        int total = ncand * npr;
        int j = lane / npr, k = lane - j * npr;
        int step_j = 64 / npr, step_k = 64 - step_j * npr;
        for (int w = lane; w < total; w += 64) {
            if (k != kr) {
                f3 v = ld3(wvi[cs.cand[j]]);
                float val = dot3(ld3(wpr[k]), v) + wpr[k][3];
                atomicMax(&cs.cmax[j], f2ord(val));
            }
            j += step_j;
            k += step_k;
            if (k >= npr) { k -= npr; j++; }
        }
        wsync();
        HPROF(28);
        bool valid = cand && ord2f(cs.cmax[slot]) <= mg;
        // the candidate set, one per lane in the oracle's list order: lanes [0, nv1) the valid incident vertices
        // in vertex order (moved there by a forward permute), then, from lane nv1 on, the incident-face edges'
        // entry / exit points and the reference-face vertices (lanes past 63 dropped, as by the oracle)
        uint64_t vm = __ballot(valid);
        int nv1 = __popcll(vm);
        int rk = __popcll(vm & ((1ull << lane) - 1ull));
        int to = valid ? rk : nv1 + (lane - rk);        // a permutation of the lanes
        f3 pt = vi - nref * (0.5f * dist);
        f3 x = mk3(__int_as_float(__builtin_amdgcn_ds_permute(to << 2, __float_as_int(pt.x))),
                   __int_as_float(__builtin_amdgcn_ds_permute(to << 2, __float_as_int(pt.y))),
                   __int_as_float(__builtin_amdgcn_ds_permute(to << 2, __float_as_int(pt.z))));
        float sv = __int_as_float(__builtin_amdgcn_ds_permute(to << 2, __float_as_int(dist)));
        bool ok = lane < nv1;
        // the incident face: the incident hull's face most anti-parallel to the reference normal (first minimum)
        float vmin = 3.0e38f;
        int ki = 1 << 20;
        for (int kk = lane; kk < npi; kk += 64) {
            float dv = dot3(ld3(wpi[kk]), nref);
            if (dv < vmin) { vmin = dv; ki = kk; }
        }
        wave_argmin(vmin, ki);
        int lpi = m.plane_loop[m.hull_plane_start[hi] + ki], lpr = m.plane_loop[m.hull_plane_start[hr] + kr];
        int li0 = lpi & 0xFFFF, lni = lpi >> 16, lr0 = lpr & 0xFFFF, lnr = lpr >> 16;
        if (c.p->narrow_phase_flags & HA_NP_NO_CLIP) lni = lnr = 0;
        f3 ni = ld3(wpi[ki]);
        float di = wpi[ki][3];
        float den = dot3(ni, nref);
        // the two face loops staged in lanes: lane j holds loop vertex j of each face and the side plane through
        // loop edge j (side_plane, the same expression for every (candidate, plane) pair), so the clipping loops
        // below read them with v_readlane instead of re-deriving them per candidate from the model's loop lists
        int rv = lane < lnr ? m.loop_v[lr0 + lane] : 0, iv = lane < lni ? m.loop_v[li0 + lane] : 0;
        f3 rsn = mk3(0, 0, 0), isn = mk3(0, 0, 0);
        float rsd = 0.0f, isd = 0.0f;
        if (lane < lnr) {
            int rv1 = m.loop_v[lr0 + (lane + 1 == lnr ? 0 : lane + 1)];
            f3 v0 = ld3(wvr[rv]);
            rsn = cross3(ld3(wvr[rv1]) - v0, nref);
            rsn = rsn * (1.0f / sqrtf(dot3(rsn, rsn)));
            rsd = -dot3(rsn, v0);
        }
        if (lane < lni) {
            int iv1 = m.loop_v[li0 + (lane + 1 == lni ? 0 : lane + 1)];
            f3 v0 = ld3(wvi[iv]);
            isn = cross3(ld3(wvi[iv1]) - v0, ni);
            isn = isn * (1.0f / sqrtf(dot3(isn, isn)));
            isd = -dot3(isn, v0);
        }
        int q = lane - nv1;
        int qe = q >> 1, qr = q - 2 * lni;
        int ivq0 = __shfl(iv, qe < 0 ? 0 : qe), ivq1 = __shfl(iv, qe + 1 >= lni ? 0 : qe + 1);
        int rvq = __shfl(rv, qr < 0 ? 0 : qr);
        // (2) lanes q < 2 lni: incident-face loop edge q / 2 clipped (Cyrus-Beck) to the reference face's side planes
        //     (through its loop edges, perpendicular to it): the entry (even q) or exit (odd q) point, when inside the
        //     segment and within the margin of the reference face
        // (3) lanes 2 lni <= q < 2 lni + lnr: reference-face loop vertex q - 2 lni projected along the reference normal
        //     onto the incident face's plane: a candidate when inside the incident face's side planes and within the
        //     margin
        // The plane loops run in wave-uniform control flow: a v_readlane of a lane's side plane inside a divergent
        // branch would read a register the allocator may reuse in that lane on the other branch
        bool isclip = q >= 0 && q < 2 * lni;
        bool isref = q >= 2 * lni && q < 2 * lni + lnr;
        f3 p0 = ld3(wvi[ivq0]), p1 = ld3(wvi[ivq1]);
        f3 r = ld3(wvr[rvq]);
        float sr = den < -1e-6f ? -(dot3(ni, r) + di) / den : 0.0f;
        f3 xr = r + nref * sr;
        float tin = 0.0f, tout = 1.0f, mx = -3.0e38f;
        bool out = false;
#pragma unroll 1
        for (int jj = 0; jj < lnr; jj++) {
            f3 sn = mk3(bcast(rsn.x, jj), bcast(rsn.y, jj), bcast(rsn.z, jj));
            float sd = bcast(rsd, jj);
            float f0 = dot3(sn, p0) + sd, f1 = dot3(sn, p1) + sd;
            if (f0 > 0.0f && f1 > 0.0f) out = true;
            else if (f0 > 0.0f) tin = fmaxf(tin, f0 / (f0 - f1));
            else if (f1 > 0.0f) tout = fminf(tout, f0 / (f0 - f1));
        }
#pragma unroll 1
        for (int jj = 0; jj < lni; jj++) {
            f3 sn = mk3(bcast(isn.x, jj), bcast(isn.y, jj), bcast(isn.z, jj));
            mx = fmaxf(mx, dot3(sn, xr) + bcast(isd, jj));
        }
        if (isclip) {
            bool ex = (q & 1) != 0;
            f3 xc = p0 + (p1 - p0) * (ex ? tout : tin);
            float dx = dot3(nref, xc) + dref;
            ok = !out && (ex ? (tout < 1.0f && tin < tout) : (tin > 0.0f && tin <= tout)) && dx <= mg;
            x = xc - nref * (0.5f * dx);
            sv = dx;
        } else if (isref) {
            ok = den < -1e-6f && sr <= mg && mx <= 0.0f;
            x = r + nref * (0.5f * sr);
            sv = sr;
        }
        HPROF(31);
        if (__ballot(ok)) {
            f3 n = refB ? nref : nref * -1.0f;
            // anchors: candidates (1) and (2) on the incident hull, (3) on the reference hull; the normal on the reference
            int nA = refB ? 0 : PCM_NORMAL_A;
            int code = (isref ? (refB ? PCM_FEAT_B : PCM_FEAT_A) : (refB ? PCM_FEAT_A : PCM_FEAT_B)) | nA;
            emit_contacts(c, ok, x, sv, n, a, b, code);
            HPROF(29);
            return;
        }
        wsync();
    }
}
#undef HPROF

// does a sphere (center c, radius r) reach the table box? Conservative for the hull inside the sphere,
// so culling with it never removes a contact the narrow phase would produce.
HD bool sphere_near_box(const float* half, PoseF Pb, f3 c, float r) {
    qf qi = qf{-Pb.q.x, -Pb.q.y, -Pb.q.z, Pb.q.w};
    f3 pl = qrot(qi, c - Pb.p);
    float dx = fmaxf(fabsf(pl.x) - half[0], 0.0f);
    float dy = fmaxf(fabsf(pl.y) - half[1], 0.0f);
    float dz = fmaxf(fabsf(pl.z) - half[2], 0.0f);
    return dx * dx + dy * dy + dz * dz <= r * r;
}
// Two unscaled hulls' oriented boxes (hull_obb: link hulls and, since round 6, every piece of a compound object),
// posed by their bodies, within the margin on all 15 axes (include/ha_obb.h, the oracle's text too): a compound pair's
// piece pair that fails it cannot touch, so its narrow phase is skipped in both. Elongated pieces (spoon, wrench,
// scissors) have loose spheres: in the C4w tail envs the boxes reject two thirds of the piece pairs the spheres keep
HD
bool piece_boxes_near(const ha_model_t& m, int h1, PoseF P1, int h2, PoseF P2, float mg) {
    float p1[3] = {P1.p.x, P1.p.y, P1.p.z}, q1[4] = {P1.q.x, P1.q.y, P1.q.z, P1.q.w};
    float p2[3] = {P2.p.x, P2.p.y, P2.p.z}, q2[4] = {P2.q.x, P2.q.y, P2.q.z, P2.q.w};
    return ha_obb_pair_near(p1, q1, m.hull_obb[h1], p2, q2, m.hull_obb[h2], mg) != 0;
}
// static k's world pose: its model pose, composed with the env's posed actor (s.sb) when the actor carries it (v14)
HD PoseF static_pose(const SimCtx& c, int k) {
    const ha_model_t& m = *c.m;
    PoseF P{ld3(m.static_pos[k]), ldq(m.static_quat[k])};
    if (m.static_posed[k]) {
        f3 bp = ld3(c.s->sb);
        qf bq = ldq(c.s->sb + 4);
        P = PoseF{bp + qrot(bq, P.p), qmul(bq, P.q)};
    }
    return P;
}
// Oriented boxes of the broad phase's box cull (pair_boxes_near): centre, orientation, half extents. A link hull's fitted
// box (hull_obb) posed by its link; a one-piece object's box (its hull's bounding box in the body frame, identity
// orientation, model.py object_box) scaled by the env's object scale and posed by the object; a static's box
// (static_half) at its pose. ha_create checks that every such hull lies inside its box.
HD void link_box(const SimCtx& c, int h, f3& bc, qf& bq, f3& hh) {
    int L = c.m->hull_link[h];
    const float* ob = c.m->hull_obb[h];
    qf lq = ldq(c.s->lq[L]);
    bc = ld3(c.s->lp[L]) + qrot(lq, ld3(ob));
    bq = qmul(lq, ldq(ob + 6));
    hh = ld3(ob + 3);
}
HD void object_box(const SimCtx& c, int o, f3& bc, qf& bq, f3& hh) {
    const float* ob = c.m->hull_obb[c.m->pool_hull[c.o[o].pool]];
    PoseF P = object_pose(c, o);
    bc = P.p + qrot(P.q, scale3(c, o, ld3(ob)));
    bq = P.q;
    hh = scale3(c, o, ld3(ob + 3));
}
HD void static_box(const SimCtx& c, int k, f3& bc, qf& bq, f3& hh) {
    PoseF P = static_pose(c, k);
    bc = P.p;
    bq = P.q;
    hh = ld3(c.m->static_half[k]);
}
// Box cull of a broad-phase candidate (kinds 1-4; lane-parallel in detect): false when the two sides' boxes are
// separated by more than the contact margin + 1 mm on one of the 15 box SAT axes (ha_obb.h ha_obb_sat, conservative;
// the 1 mm covers the rounding of the posed boxes). Their hulls are then apart too and the narrow phase would emit nothing (nor write a
// persistent-manifold record: pcm_commit writes none for an empty manifold); the oracle has no such cull and runs the
// narrow phase, which finds the same empty result. Compound objects (several pieces) are not culled here
HD bool pair_boxes_near(const SimCtx& c, int kind, int A, int B, float mg) {
    const ha_model_t& m = *c.m;
    if (kind <= 3 && m.pool_nhull[c.o[A].pool] != 1) return true;
    if (kind == 2 && m.pool_nhull[c.o[B].pool] != 1) return true;
    f3 ca, cb, ha, hb;
    qf qa, qb;
    if (kind == 4) link_box(c, A, ca, qa, ha);
    else object_box(c, A, ca, qa, ha);
    if (kind == 1 || kind == 4) static_box(c, B, cb, qb, hb);
    else if (kind == 2) object_box(c, B, cb, qb, hb);
    else link_box(c, B, cb, qb, hb);
    // the posed boxes as ha_obb.h records (centre, half, quat) at the origin, then its 15-axis test
    float ra[12] = {0.0f, 0.0f, 0.0f, ha.x, ha.y, ha.z, qa.x, qa.y, qa.z, qa.w, 0.0f, 0.0f};
    float rb[12] = {0.0f, 0.0f, 0.0f, hb.x, hb.y, hb.z, qb.x, qb.y, qb.z, qb.w, 0.0f, 0.0f};
    const float id[4] = {0.0f, 0.0f, 0.0f, 1.0f};
    float pa[3] = {ca.x, ca.y, ca.z}, pb[3] = {cb.x, cb.y, cb.z};
    float xa[3], Ra[9], xb[3], Rb[9];
    ha_obb_world(pa, id, ra, xa, Ra);
    ha_obb_world(pb, id, rb, xb, Rb);
    return ha_obb_sat(xa, Ra, ra + 3, xb, Rb, rb + 3, mg + 1e-3f) != 0;
}

// pair enumeration in the oracle's order (see detect() in physics_oracle.c)
// pair p -> (kind, A, B): kinds 0 object-ground, 1 object-static B, 2 object-object, 3 link hull B - object,
// 4 link hull A - static B; then (detect's self-pair pass) 5: self-collision pair A of the model (v12 self_pair)
HD bool pair_desc(const SimCtx& c, int p, int& kind, int& A, int& B) {
    int NO = c.NO, NLH = c.m->n_link_hulls, NS = c.m->n_static;
    for (int o = 0; o < NO; o++) {
        int n = 1 + NS + (NO - 1 - o) + NLH;
        if (p < n) {
            A = o;
            if (p == 0) { kind = 0; B = -1; }
            else if (p < 1 + NS) { kind = 1; B = p - 1; }
            else if (p < 1 + NS + (NO - 1 - o)) { kind = 2; B = o + 1 + (p - 1 - NS); }
            else { kind = 3; B = p - 1 - NS - (NO - 1 - o); }
            return true;
        }
        p -= n;
    }
    if (p < NLH * NS) { kind = 4; A = p / NS; B = p - A * NS; return true; }
    return false;
}

// ----------------------------------------------------------------------------- hierarchical broad phase (round 6)
// Most of the enumeration above is link-hull pairs (C5: 176 object-link and 132 link-static of 392), and in a bin
// scene nearly all of them fail the sphere / box tests. Before the 64-pair batches, detect() bounds the link hulls
// in quads (hulls 4g .. 4g+3, one DPP quad of lanes): centre C_g = the mean of the quad's hull centres, radius R_g =
// max_k (|c_k - C_g| + r_k). A pair (object o, hull k) passes the sphere test only if |c_o - c_k| <= r_o + r_k + mg,
// and then |c_o - C_g| <= r_o + R_g + mg (triangle inequality); a link-static pair passes the box test only if the
// box distance of c_k is <= r_k + mg, and the box distance is 1-Lipschitz, so that of C_g is <= R_g + mg. The quad
// tests (with 0.1% + 1 mm of slack over float rounding) therefore reject only pairs the per-pair tests reject, and
// the batches run over the pairs of the quads that pass, in the enumeration's order with their enumeration index
// (record slots, face records): the contacts, their order and every record are those of the flat enumeration,
// which the oracle keeps. om: bit o*G + g = object o near quad g; sm: bit g*NS + b = static b near quad g.
HD int quad_hulls(uint32_t g, int G, int NLH) {
    return 4 * __builtin_popcount(g) - (int)((g >> (G - 1)) & 1u) * (4 * G - NLH);
}
// the t-th hull of the quads set in g
HD int quad_hull(uint32_t g, int t, int NLH) {
    for (int q = 0; g; q++, g >>= 1) {
        if (!(g & 1u)) continue;
        int nh = min(4, NLH - 4 * q);
        if (t < nh) return 4 * q + t;
        t -= nh;
    }
    return -1;
}
// pair r of the culled enumeration: its kind / sides, and p = its index in the flat one (pair_desc)
HD bool pair_compact(const SimCtx& c, int G, uint64_t om, uint64_t sm, int& p, int& kind, int& A, int& B) {
    int NO = c.NO, NLH = c.m->n_link_hulls, NS = c.m->n_static;
    int r = p, orig = 0;
    uint32_t gm = (1u << G) - 1u;
    for (int o = 0; o < NO; o++) {
        int head = 1 + NS + (NO - 1 - o);
        uint32_t g = (uint32_t)(om >> (o * G)) & gm;
        int nl = quad_hulls(g, G, NLH);
        if (r < head + nl) {
            A = o;
            if (r == 0) { kind = 0; B = -1; }
            else if (r < 1 + NS) { kind = 1; B = r - 1; }
            else if (r < head) { kind = 2; B = o + 1 + (r - 1 - NS); }
            else { kind = 3; B = quad_hull(g, r - head, NLH); }
            p = orig + (kind == 3 ? head + B : r);
            return true;
        }
        r -= head + nl;
        orig += head + NLH;
    }
    uint32_t bm = (1u << NS) - 1u;
    for (int q = 0; q < G; q++) {
        uint32_t s = (uint32_t)(sm >> (q * NS)) & bm;
        int pc = __builtin_popcount(s), cnt = min(4, NLH - 4 * q) * pc;
        if (r < cnt) {
            int h = r / pc, k = r - h * pc;
            for (; k > 0; k--) s &= s - 1u;
            kind = 4; A = 4 * q + h; B = __builtin_ctz(s);
            p = orig + A * NS + B;
            return true;
        }
        r -= cnt;
    }
    return false;
}
// the quads' object / static masks and the culled pair count (G quads; G * NO <= 64, G * NS <= 64)
HD void broad_quads(const SimCtx& c, int G, uint64_t& om, uint64_t& sm, int& neff) {
    const EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int lane = c.lane, NO = c.NO, NLH = m.n_link_hulls, NS = m.n_static;
    float mg = c.p->contact_margin;
    bool hv = lane < NLH;
    f3 ch = mk3(0.0f, 0.0f, 0.0f);
    float rk = 0.0f;
    if (hv) {
        int Lk = m.hull_link[lane];
        ch = ld3(s.lp[Lk]) + qrot(ldq(s.lq[Lk]), ld3(m.hull_center[lane]));
        rk = m.hull_radius[lane];
    }
    f3 C = ch;
    C.x += dpp_f<0xB1>(C.x); C.y += dpp_f<0xB1>(C.y); C.z += dpp_f<0xB1>(C.z);
    C.x += dpp_f<0x4E>(C.x); C.y += dpp_f<0x4E>(C.y); C.z += dpp_f<0x4E>(C.z);
    C = C * (1.0f / (float)max(1, min(4, NLH - (lane & ~3))));
    f3 dc = ch - C;
    float d = hv ? sqrtf(dot3(dc, dc)) + rk : 0.0f;
    d = fmaxf(d, dpp_f<0xB1>(d));
    d = fmaxf(d, dpp_f<0x4E>(d));
    float R = d * 1.001f + mg + 1.0e-3f;
    // statics near each quad (every lane of a quad holds its sphere; lane 4g's bits are read)
    uint32_t sb = 0;
    for (int b = 0; b < NS; b++)
        if (sphere_near_box(m.static_half[b], static_pose(c, b), C, R)) sb |= 1u << b;
    // quads near each object (lane o; an object with collisions off has no candidate pairs)
    f3 co = mk3(0.0f, 0.0f, 0.0f);
    float ro = -1.0e30f;
    if (lane < NO && c.o[lane].coll != 0) {
        int pa = c.o[lane].pool;
        PoseF Po = object_pose(c, lane);
        co = Po.p + qrot(Po.q, scale3(c, lane, ld3(m.pool_center[pa])));
        ro = scale_radius(c, lane, m.pool_radius[pa]);
    }
    uint32_t ob = 0;
    sm = 0;
    neff = 0;
    for (int q = 0; q < G; q++) {
        f3 Cq = mk3(bcast(C.x, 4 * q), bcast(C.y, 4 * q), bcast(C.z, 4 * q));
        float rr = (ro + bcast(R, 4 * q)) * 1.0001f;
        f3 dq = co - Cq;
        if (ro > -1.0e29f && dot3(dq, dq) <= rr * rr) ob |= 1u << q;
        uint32_t sq = (uint32_t)bcast_i((int)sb, 4 * q);
        sm |= (uint64_t)sq << (q * NS);
        neff += min(4, NLH - 4 * q) * __builtin_popcount(sq);
    }
    om = 0;
    for (int o = 0; o < NO; o++) {
        uint32_t g = (uint32_t)bcast_i((int)ob, o);
        om |= (uint64_t)g << (o * G);
        neff += 1 + NS + (NO - 1 - o) + quad_hulls(g, G, NLH);
    }
}
// the two link hulls of self-collision pair k
HD void self_pair_hulls(const ha_model_t& m, int k, int& ha, int& hb) {
    uint32_t sp = m.self_pair[k];
    ha = (int)(sp & 255u);
    hb = (int)(sp >> 8);
}

// ----------------------------------------------------------------------------- persistent contact manifolds (v13)
// PhysX keeps a pair's contact manifold across substeps (persistent contact manifolds, PCM; inferred, its source is
// closed) and refreshes its points from the bodies' current poses while their relative motion stays small. Here a
// record per candidate pair (ha_state_t.contact_cache, slot = the pair's index in detect's enumeration, then the self
// pairs) holds the manifold a narrow phase emitted: the relative pose it was built at, and per point the point on each
// body in that body's frame and the normal in side B's frame. The oracle restates every expression (pcm_store,
// pcm_refresh in physics_oracle.c), so results stay bit-identical.
//
// Side A / side B body poses and body codes of candidate pair (kind, A, B): the sides narrow_phase gives collide_hulls
// (UNIFORM: the pair is wave-uniform and its object poses read the pool id through an SGPR; false: a per-lane pair)
template <bool UNIFORM = true>
HD void pair_bodies(const SimCtx& c, int kind, int A, int B, PoseF& PA, PoseF& PB, int& a, int& b) {
    const EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    auto opose = [&](int o) { return UNIFORM ? object_pose_u(c, o) : object_pose(c, o); };
    if (kind <= 2) {
        PA = opose(A);
        a = A;
        if (kind == 0) { PB = PoseF{mk3(0, 0, 0), qf{0, 0, 0, 1}}; b = -1; }    // the ground plane z = 0
        else if (kind == 1) { PB = static_pose(c, B); b = -1; }
        else { PB = opose(B); b = B; }
    } else if (kind == 3) {
        int Lk = m.hull_link[B];
        PA = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])};
        a = 100 + Lk;
        PB = opose(A);
        b = A;
    } else if (kind == 4) {
        int Lk = m.hull_link[A];
        PA = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])};
        a = 100 + Lk;
        PB = static_pose(c, B);
        b = -1;
    } else {                                    // self pair A: hull b on side A, hull a on side B
        int ha_, hb_;
        self_pair_hulls(m, A, ha_, hb_);
        int La = m.hull_link[ha_], Lb = m.hull_link[hb_];
        PA = PoseF{ld3(s.lp[Lb]), ldq(s.lq[Lb])};
        a = 100 + Lb;
        PB = PoseF{ld3(s.lp[La]), ldq(s.lq[La])};
        b = 100 + La;
    }
}
HD qf qconj(qf q) { return qf{-q.x, -q.y, -q.z, q.w}; }

// The record of the running pair's manifold (c.pslot), from the points emit_contacts staged: lane t < k its point on
// A (x + n sep / 2) in A's frame, its point on B (x - n sep / 2) in B's frame, its normal in the frame of the body that
// carries it and its anchor; lane 0 the relative pose and k. Vector stores: every record access of the kernel is a
// per-lane vector access
HD void pcm_commit(SimCtx& c) {
    int k = c.pemit;
    c.pemit = 0;
    if (c.pslot < 0 || k <= 0) return;
    wsync();
    PoseF PA, PB;
    int a_, b_;
    pair_bodies(c, c.pkind, c.pA, c.pB, PA, PB, a_, b_);
    float* rec = c.pcm + (size_t)c.pslot * HA_PCM_REC;
    qf qbc = qconj(PB.q);
    int t = c.lane < k ? c.lane : -1;
    if (t >= 0) {
        const float* q = reinterpret_cast<const float*>(c.col.cand) + 8 * t;
        f3 x = mk3(q[0], q[1], q[2]), n = mk3(q[3], q[4], q[5]);
        float sep = q[6];
        int code = __float_as_int(q[7]);
        float hs = 0.5f * sep;
        qf qac = qconj(PA.q);
        f3 la = qrot(qac, (x + n * hs) - PA.p);
        f3 lb = qrot(qbc, (x - n * hs) - PB.p);
        f3 ln = qrot((code & PCM_NORMAL_A) ? qac : qbc, n);
        float* r = rec + 8 + 9 * t;
        st3(r, la);
        st3(r + 3, lb);
        st3(r + 6, ln);
        rec[44 + t] = (float)code;
    }
    if (c.lane == 0) {
        st3(rec, qrot(qbc, PA.p - PB.p));
        rec[3] = (float)k;
        stq(rec + 4, qmul(qbc, PA.q));
    }
}

// already-reduced points (lanes in order, valid ones only) into the contact list: the refreshed manifold of a record
HD void emit_points(SimCtx& c, bool valid, f3 pt, float sep, f3 n, int a, int b) {
    EnvLDS& s = *c.s;
    int lane = c.lane;
    uint64_t vm = __ballot(valid);
    int k = __popcll(vm);
    if (k == 0) return;
    int nc0 = s.nc;
    if (nc0 + k <= c.maxc) {
        count_offered(c, k, a, b);
        if (lane == 0) s.nc = nc0 + k;
        if (valid) ct_put(c, nc0 + __popcll(vm & ((1ull << lane) - 1ull)), pt, n, sep, a, b);
        wsync();
        return;
    }
    f3 P[4], N[4];
    float S[4];
    int CD[4] = {0, 0, 0, 0};           // (the list path does not read the anchors)
    uint64_t mk = vm;
#pragma unroll
    for (int t = 0; t < 4; t++) {
        int src = mk ? __ffsll((unsigned long long)mk) - 1 : 0;
        mk &= mk - 1;
        P[t] = mk3(bcast(pt.x, src), bcast(pt.y, src), bcast(pt.z, src));
        N[t] = mk3(bcast(n.x, src), bcast(n.y, src), bcast(n.z, src));
        S[t] = bcast(sep, src);
    }
    store_chosen(c, k, P, N, S, CD, a, b);
}

// Pair slot `slot`'s record test (the oracle's pcm_refresh): it applies when it holds points and the pair's relative
// pose (A's body in B's frame) is within pcm_lin_tol / pcm_cos_tol of the pose it was built at. Evaluated per lane for a
// whole batch of candidate pairs at once (the broad phase's batch, or the first 64 self-pair candidates), so a pair whose
// record does not apply costs no load latency of its own. The header comes in two 16-byte loads per lane
HD bool pcm_valid_lane(const SimCtx& c, int slot, int kind, int A, int B) {
    const ha_params_t& p = *c.p;
    const float4* h = reinterpret_cast<const float4*>(c.pcm + (size_t)slot * HA_PCM_REC);
    float4 h0 = h[0], h1 = h[1];
    if ((int)h0.w <= 0) return false;
    PoseF PA, PB;
    int a_, b_;
    pair_bodies<false>(c, kind, A, B, PA, PB, a_, b_);
    qf qbc = qconj(PB.q);
    f3 d = qrot(qbc, PA.p - PB.p) - mk3(h0.x, h0.y, h0.z);
    float lt = p.pcm_lin_tol;
    if (dot3(d, d) > lt * lt) return false;
    qf qr = qmul(qbc, PA.q);
    float cq = ((qr.x * h1.x + qr.y * h1.y) + qr.z * h1.z) + qr.w * h1.w;
    return !(fabsf(cq) < p.pcm_cos_tol);
}
// one record in one register: lane i < HA_PCM_REC holds word i (a 192-byte coalesced load, issued a pair ahead)
HD float pcm_load(const SimCtx& c, int slot) {
    return c.lane < HA_PCM_REC ? c.pcm[(size_t)slot * HA_PCM_REC + c.lane] : 0.0f;
}
// A pair whose record applies (pcm_valid_lane): every point is re-evaluated from the current poses - the surface points
// carried by their bodies, the normal by the body that owns it, the separation along the normal, the point half the
// separation off its feature - those within the contact margin go to the list in record order, and the pair needs no
// narrow phase. rv = the record (pcm_load); lane t < k gathers its point's words by lane permutes
HD void pcm_emit_record(SimCtx& c, float rv, int kind, int A, int B) {
    const ha_params_t& p = *c.p;
    int lane = c.lane;
    int k = (int)bcast(rv, 3);
    PoseF PA, PB;
    int a, b;
    pair_bodies(c, kind, A, B, PA, PB, a, b);
    int t = lane < 4 ? lane : 0;
    float r[9];
#pragma unroll
    for (int f = 0; f < 9; f++) r[f] = __shfl(rv, 8 + 9 * t + f);
    int code = (int)__shfl(rv, 44 + t);
    bool valid = false;
    f3 x = mk3(0, 0, 0), n = mk3(0, 0, 0);
    float sp = 0.0f;
    if (lane < k && lane < 4) {
        f3 wa = PA.p + qrot(PA.q, mk3(r[0], r[1], r[2]));
        f3 wb = PB.p + qrot(PB.q, mk3(r[3], r[4], r[5]));
        n = qrot((code & PCM_NORMAL_A) ? PA.q : PB.q, mk3(r[6], r[7], r[8]));
        sp = dot3(n, wa - wb);
        valid = sp <= p.contact_margin;
        int f = code & 3;
        x = f == PCM_FEAT_A ? wa - n * (0.5f * sp) : (f == PCM_FEAT_B ? wb + n * (0.5f * sp) : (wa + wb) * 0.5f);
    }
    emit_points(c, valid, x, sp, n, a, b);
    if (lane == 0) c.s->cst[5] += 1;
}

// piece pairs of a candidate pair (1 unless an object is a compound of several convex pieces)
HD int pair_pieces(const SimCtx& c, int kind, int A, int B) {
    const ha_model_t& m = *c.m;
    if (kind >= 4) return 1;
    int n = m.pool_nhull[upool(c, A)];
    if (kind == 2) n *= m.pool_nhull[upool(c, B)];
    return n;
}

// Compound pairs (kinds 2, 3; round 6): which of piece pairs j0 .. j0 + 63 can touch. Lane t tests piece pair j0 + t:
// the two pieces' own spheres, then (unscaled bodies) their oriented boxes (piece_boxes_near); PhysX's broad phase
// sees each convex shape of an actor on its own. The oracle tests each piece pair the same way before its narrow phase
// (physics_oracle.c detect). A block of its own that derives everything from the pair's indices again, so that none of
// its values stay live into the narrow phases (VGPRs); the result is one 64-bit mask (SGPRs)
HD uint64_t piece_mask(const SimCtx& c, int kind, int A, int B, int j0, int np) {
    const EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int jj = j0 + c.lane;
    bool near = false;
    if (jj < np) {
        int ho = m.pool_hull[upool(c, A)];
        float mg = c.p->contact_margin;
        int h1, h2, b1, b2;
        PoseF P1, P2;
        f3 c1;
        float r1;
        if (kind == 2) {
            int pb = upool(c, B), n2 = m.pool_nhull[pb];
            int j1 = jj / n2;
            h1 = ho + j1; h2 = m.pool_hull[pb] + (jj - j1 * n2);
            P1 = object_pose_u(c, A); P2 = object_pose_u(c, B); b1 = A; b2 = B;
            c1 = P1.p + qrot(P1.q, scale3(c, A, ld3(m.hull_center[h1])));
            r1 = scale_radius(c, A, m.hull_radius[h1]);
        } else {
            int Lk = m.hull_link[B];
            h1 = B; P1 = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; b1 = -1;
            h2 = ho + jj; P2 = object_pose_u(c, A); b2 = A;
            c1 = P1.p + qrot(P1.q, ld3(m.hull_center[B]));
            r1 = m.hull_radius[B];
        }
        f3 c2 = P2.p + qrot(P2.q, scale3(c, b2, ld3(m.hull_center[h2])));
        float rr = r1 + scale_radius(c, b2, m.hull_radius[h2]) + mg;
        f3 dc = c1 - c2;
        near = dot3(dc, dc) <= rr * rr;
#ifndef HA_X_NO_PIECE_BOX      /* A/B timing builds only (the oracle keeps the box test): the piece spheres alone */
        if (near && !body_scaled(c, b1) && !body_scaled(c, b2)) near = piece_boxes_near(m, h1, P1, h2, P2, mg);
#endif
    }
    return __ballot(near);
}

// narrow phase of piece pair j of candidate pair (kind, A, B): the two sides' hulls, poses and body codes
HD void narrow_phase(SimCtx& c, int kind, int A, int B, int j) {
    const EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    if (kind == 0) {
        if (c.lane == 0) c.s->cst[6] += 1;
        collide_ground(c, m.pool_hull[upool(c, A)] + j, object_pose_u(c, A), A);
        return;
    }
    int h1, h2, b1, b2, k2;
    PoseF P1, P2;
    if (kind <= 3) {
        // the objects of the pair: A on side A (kinds 1, 2), and the object on side B (kind 2: B, kind 3: A), posed by
        // one call each, so that the branches below only pick values (the branches share no look-alike calls)
        int pa = upool(c, A), ho = m.pool_hull[pa];
        int ob = kind == 2 ? B : A;
        int pb = upool(c, ob), n2 = m.pool_nhull[pb];
        PoseF Po = object_pose_u(c, A);
        PoseF Pb = object_pose_u(c, ob);
        if (kind == 1) {
            h1 = ho + j; P1 = Po; b1 = A; h2 = m.static_hull[B]; P2 = static_pose(c, B); b2 = -1; k2 = -100 - B;
            // the piece's own sphere against the exact box (the oracle's per-piece near_box; for a one-hull object
            // the broad phase's test again)
            f3 cp = Po.p + qrot(Po.q, scale3(c, A, ld3(m.hull_center[h1])));
            if (!sphere_near_box(m.static_half[B], P2, cp, scale_radius(c, A, m.hull_radius[h1]) + c.p->contact_margin))
                return;
        } else if (kind == 2) {
            int j1 = j / n2;
            h1 = ho + j1; P1 = Po; b1 = A; h2 = m.pool_hull[pb] + (j - j1 * n2); P2 = Pb; b2 = B; k2 = B;
        } else {
            int Lk = m.hull_link[B];
            h1 = B; P1 = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; b1 = 100 + Lk; h2 = ho + j; P2 = Pb; b2 = A; k2 = A;
        }
    } else if (kind == 4) {
        int Lk = m.hull_link[A];
        h1 = A; P1 = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; b1 = 100 + Lk; h2 = m.static_hull[B];
        P2 = static_pose(c, B); b2 = -1; k2 = -100 - B;
    } else {
        // self-collision pair (a, b), a < b: hull b on side A, hull a on side B (normal from a to b). Consecutive pairs
        // share hull a, so side B's world vertices / planes stay in the scratch and a pair whose side-A sphere clears one
        // of a's planes never sets up side A
        int ha_, hb_;
        self_pair_hulls(m, A, ha_, hb_);
        int La = m.hull_link[ha_], Lb = m.hull_link[hb_];
        h1 = hb_; P1 = PoseF{ld3(s.lp[Lb]), ldq(s.lq[Lb])}; b1 = 100 + Lb;
        h2 = ha_; P2 = PoseF{ld3(s.lp[La]), ldq(s.lq[La])}; b2 = 100 + La; k2 = b2;
    }
    if (c.lane == 0) c.s->cst[6] += 1;         // contact_stats: hull-pair narrow phases run (diagnostics)
    collide_hulls(c, h1, P1, h2, P2, b1, b2, b1, k2);
}

// a compound pair's gathered points (lane = point, in gather order) -> one manifold of <= 4 contacts
HD void gather_emit(SimCtx& c, int kind, int A, int B) {
    EnvLDS& s = *c.s;
    const ColView& cs = c.col;
    wsync();
    int lane = c.lane;
    bool valid = lane < s.ng;
    f3 pt = mk3(0, 0, 0), n = mk3(0, 0, 0);
    float sep = 0;
    int code = 0;
    if (valid) {
        pt = ld3(cs.gp[lane]);
        sep = cs.gp[lane][3];
        n = ld3(cs.gn[lane]);
        code = __float_as_int(cs.gn[lane][3]);
    }
    int a = kind == 3 ? 100 + c.m->hull_link[B] : A;
    int b = kind == 2 ? B : (kind == 3 ? A : -1);
    emit_contacts(c, valid, pt, sep, n, a, b, code);
}

// self-collision pass (ha_model_t v12; after every other pair, the oracle's order):
//  1. the link hulls' world boxes (lane = hull, include/ha_obb.h ha_obb_world) and their circumscribed radii into the
//     narrow-phase scratch, component-major (lanes reading different hulls read consecutive words);
//  2. one lane per pair tests the two spheres (ha_obb_spheres_near); the pairs that pass are compacted, in pair order,
//     and one lane per such pair runs the 15 SAT axes (ha_obb_sat) - the oracle's ha_obb_near, split so that the
//     axis tests run on full waves. The candidate bits go to the env's LDS bit set (the narrow phases below overwrite the
//     scratch), and the first 64 candidates' records are loaded into a register at once;
//  3. per candidate, in pair order: if the pair's last narrow phase ended on a separating face (the env's per-pair
//     byte in its global area), that one face is tested first, with the narrow phase's own expressions (world plane,
//     the other hull's world vertices, min): still separating by more than the margin means the full narrow phase
//     would stop on a face too (its SAT maximises over every face), so the pair is skipped with the same result.
//     The record is a hint only: results never depend on it (the oracle has none);
//  4. otherwise the hull narrow phase, which records the separating face for the next substep.
HD void detect_self(SimCtx& c, int npairs) {
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int lane = c.lane, NLH = m.n_link_hulls, nsp = m.n_self_pairs;
    float mg = c.p->contact_margin;
    float* tab = reinterpret_cast<float*>(c.col.wvA);        // tab[comp NLH + hull]: centre 3, R 9, half 3, radius
    uint16_t* spl = reinterpret_cast<uint16_t*>(tab + 16 * NLH);     // pairs whose spheres are near
    uint16_t* cdl = spl + nsp;                                       // the first 64 candidates
#ifdef HA_PROFILE
    unsigned long long _s0 = __builtin_amdgcn_s_memtime();
#endif
    if (lane < NLH) {
        int L = m.hull_link[lane];
        float w[15];
        ha_obb_world(s.lp[L], s.lq[L], m.hull_obb[lane], w, w + 3);
        w[12] = m.hull_obb[lane][3]; w[13] = m.hull_obb[lane][4]; w[14] = m.hull_obb[lane][5];
        for (int i = 0; i < 15; i++) tab[i * NLH + lane] = w[i];
        tab[15 * NLH + lane] = ha_obb_radius(w + 12);
    }
    if (lane < HA_MAX_SELF_PAIRS / 32) c.selfm[lane] = 0u;
    c.colA_h = c.colB_h = -1;           // the box table overwrote the cached hull sides
    c.colA_p = false;
    wsync();
    const uint64_t below = (1ull << lane) - 1ull;
    int nsl = 0;
#pragma unroll 1
    for (int base = 0; base < nsp; base += 64) {
        int p = base + lane;
        bool near = false;
        if (p < nsp) {
            int h1, h2;
            self_pair_hulls(m, p, h1, h2);
            float ca[3] = {tab[h1], tab[NLH + h1], tab[2 * NLH + h1]};
            float cb[3] = {tab[h2], tab[NLH + h2], tab[2 * NLH + h2]};
            near = ha_obb_spheres_near(ca, tab[15 * NLH + h1], cb, tab[15 * NLH + h2], mg) != 0;
        }
        uint64_t mk = __ballot(near);
        if (near) spl[nsl + __popcll(mk & below)] = (uint16_t)p;
        nsl += __popcll(mk);
    }
    wsync();
    int ncd = 0;
#pragma unroll 1
    for (int base = 0; base < nsl; base += 64) {
        int i = base + lane, p = 0;
        bool cand = false;
        if (i < nsl) {
            p = spl[i];
            int h1, h2;
            self_pair_hulls(m, p, h1, h2);
            float A[15], B[15];
            for (int q = 0; q < 15; q++) { A[q] = tab[q * NLH + h1]; B[q] = tab[q * NLH + h2]; }
            cand = ha_obb_sat(A, A + 3, A + 12, B, B + 3, B + 12, mg) != 0;
        }
        uint64_t mk = __ballot(cand);
        if (cand) {
            atomicOr(&c.selfm[p >> 5], 1u << (p & 31));
            int r = ncd + __popcll(mk & below);
            if (r < 64) cdl[r] = (uint16_t)p;
        }
        ncd += __popcll(mk);
    }
    wsync();
    // the records of the first 64 candidates (in pair order, the order of the loop below), one load for all; and the
    // point counts of their persistent manifolds (slot npairs + pair)
    int crec = 0xFF;
    if (c.selfc && lane < ncd) crec = c.selfc[cdl[lane]];
    // the first 64 candidates whose persistent-manifold record applies (lane = candidate rank), tested at once; their
    // records are loaded a candidate ahead
    // (in a block of its own before the candidate loop, so that none of its values stay live into the narrow phases)
    bool pv = false;
    if (c.pcm && lane < ncd) pv = pcm_valid_lane(c, npairs + cdl[lane], 5, cdl[lane], -1);
    uint64_t vmask = __ballot(pv);
    asm volatile("" : "+s"(vmask));
#ifdef HA_PROFILE
    PROF_COUNT(83, __builtin_amdgcn_s_memtime() - _s0);              // box table + box tests
#endif
    int rank = 0;
#pragma unroll 1
    for (int w32 = 0; w32 < (nsp + 31) >> 5; w32++) {
        uint32_t mask = c.selfm[w32];
#pragma unroll 1
        while (mask) {
            int bit = __ffs(mask) - 1;
            mask &= mask - 1;
            int k = __builtin_amdgcn_readfirstlane(32 * w32 + bit);
            int h1, h2;
            self_pair_hulls(m, k, h1, h2);
            int La = m.hull_link[h1], Lb = m.hull_link[h2];
#ifdef HA_PROFILE
            unsigned long long _r0 = __builtin_amdgcn_s_memtime();
            PROF_COUNT(85, 1);                                              // candidates
#endif
            int rec;
            bool refresh = false;
            if (rank < 64) {
                rec = __builtin_amdgcn_readlane(crec, rank);
                refresh = (vmask >> rank) & 1ull;
            } else {
                rec = __builtin_amdgcn_readfirstlane(c.selfc ? (int)c.selfc[k] : 0xFF);
            }
            c.pslot = -1;
            if (c.pcm) {
                // the pair's persistent manifold first (it decides the pair's contacts); then the separating-face record
#ifdef HA_PROFILE
                unsigned long long _q0 = __builtin_amdgcn_s_memtime();
#endif
                // (past the first 64 candidates: the same test in turn, on every lane)
                if (rank >= 64) refresh = __ballot(pcm_valid_lane(c, npairs + k, 5, k, -1)) != 0ull;
                if (refresh) pcm_emit_record(c, pcm_load(c, npairs + k), 5, k, -1);
#ifdef HA_PROFILE
                wsync();
                PROF_COUNT(88, __builtin_amdgcn_s_memtime() - _q0);
                PROF_COUNT(89, refresh);
#endif
                rank++;
                if (refresh) continue;
                c.pslot = npairs + k; c.pkind = 5; c.pA = k; c.pB = -1;
            } else {
                rank++;
            }
#ifdef HA_PROFILE
            PROF_COUNT(86, rec != 0xFF);                                    // candidates with a record
#endif
            if (rec != 0xFF) {
                // the recorded face (side B: hull a = h1, side A: hull b = h2) against the other hull's vertices
                bool fb = (rec & 0x80) != 0;
                int hf = fb ? h1 : h2, hv = fb ? h2 : h1, kf = rec & 0x7F;
                int Lf = fb ? La : Lb, Lv = fb ? Lb : La;
                if (kf < m.hull_nplanes[hf]) {
                    PoseF PF = PoseF{ld3(s.lp[Lf]), ldq(s.lq[Lf])}, PV = PoseF{ld3(s.lp[Lv]), ldq(s.lq[Lv])};
                    f3 n;
                    float d;
                    world_plane(m, hf, kf, PF, false, mk3(1, 1, 1), n, d);
                    float v = 3.0e38f;
                    if (lane < m.hull_nverts[hv]) v = dot3(n, PV.p + qrot(PV.q, ld3(m.verts[m.hull_vert_start[hv] + lane]))) + d;
                    bool skip = wave_min(v) > mg;
#ifdef HA_PROFILE
                    wsync();
                    PROF_COUNT(84, __builtin_amdgcn_s_memtime() - _r0);    // record checks
                    PROF_COUNT(87, skip);                                   // skipped by their record
#endif
                    if (skip) continue;                     // separated on that face, as the narrow phase would find
                }
            }
#ifdef HA_X_SELF_NO_NARROW    /* A/B timing builds only: the self pass without its narrow phases */
            continue;
#endif
#ifdef HA_PROFILE
            c.pk = 5;
            unsigned long long _k0 = __builtin_amdgcn_s_memtime();
            int _nc0 = s.nc;
#endif
#ifdef HA_X_SELF_DRY      /* A/B timing builds only: self narrow phases that emit no contacts */
            c.dry = true;
#endif
            narrow_phase(c, 5, k, -1, 0);
#ifdef HA_X_SELF_DRY
            c.dry = false;
#endif
            pcm_commit(c);
            c.pslot = -1;
            if (c.selfc && lane == 0 && c.sepf != rec) c.selfc[k] = (uint8_t)c.sepf;
#ifdef HA_PROFILE
            wsync();
            PROF_COUNT(80, __builtin_amdgcn_s_memtime() - _k0);          // self pairs: time / pairs / with contacts
            PROF_COUNT(81, 1);
            PROF_COUNT(82, s.nc != _nc0);
#endif
        }
    }
    wsync();
}

// The separating-face record of a one-piece candidate pair (PhysCfg off_pairf): the face its last narrow phase ended on
// (bit 7 set: a face of side B's hull, else of side A's; the low 7 bits its plane) against the other side's world
// vertices at the current poses, with the narrow phase's own expressions (world_plane, the posed vertices, dot + d).
// Separated by more than the margin, the hull SAT would end on a face as well and the pair has no contacts: skipping it
// changes no result (the oracle has no record and runs the narrow phase). Sides as narrow_phase gives them
HD bool sep_face_skip(const SimCtx& c, int kind, int A, int B, int rec) {
    const EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int h1, h2, b1, b2;
    PoseF P1, P2;
    if (kind == 1) {
        h1 = m.pool_hull[upool(c, A)]; P1 = object_pose_u(c, A); b1 = A;
        h2 = m.static_hull[B]; P2 = static_pose(c, B); b2 = -1;
    } else if (kind == 2) {
        h1 = m.pool_hull[upool(c, A)]; P1 = object_pose_u(c, A); b1 = A;
        h2 = m.pool_hull[upool(c, B)]; P2 = object_pose_u(c, B); b2 = B;
    } else if (kind == 3) {
        int Lk = m.hull_link[B];
        h1 = B; P1 = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; b1 = 100 + Lk;
        h2 = m.pool_hull[upool(c, A)]; P2 = object_pose_u(c, A); b2 = A;
    } else {
        int Lk = m.hull_link[A];
        h1 = A; P1 = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; b1 = 100 + Lk;
        h2 = m.static_hull[B]; P2 = static_pose(c, B); b2 = -1;
    }
    bool fb = (rec & 0x80) != 0;
    int kf = rec & 0x7F;
    int hf = fb ? h2 : h1, hv = fb ? h1 : h2, bf = fb ? b2 : b1, bv = fb ? b1 : b2;
    PoseF PF = fb ? P2 : P1, PV = fb ? P1 : P2;
    if (kf >= m.hull_nplanes[hf]) return false;
    f3 n;
    float d;
    world_plane(m, hf, kf, PF, body_scaled(c, bf), inv_scale(c, bf), n, d);
    float v = 3.0e38f;
    if (c.lane < m.hull_nverts[hv])
        v = dot3(n, PV.p + qrot(PV.q, scale3(c, bv, ld3(m.verts[m.hull_vert_start[hv] + c.lane])))) + d;
    return wave_min(v) > c.p->contact_margin;
}

template <bool SELF>
HD void detect(SimCtx& c) {
    EnvLDS& s = *c.s;
    const ha_model_t& m = *c.m;
    int lane = c.lane;
    if (lane == 0) { s.nc = 0; s.noff = 0; }
    c.colA_h = c.colB_h = -1;       // poses changed since the last detect(): no cached hull sides
    c.colA_p = false;
    c.colA_b = c.colB_b = -1000;
    int NO = c.NO, NLH = m.n_link_hulls, NS = m.n_static;
    int npairs = 0;
    for (int o = 0; o < NO; o++) npairs += 1 + NS + (NO - 1 - o) + NLH;
    npairs += NLH * NS;
    wsync();
    // the quad cull (above pair_compact) where the flat enumeration takes more than one batch
    int G = (NLH + 3) >> 2, neff = npairs;
    uint64_t om = 0, sm = 0;
    // (the Allegro scenes' enumerations fit one batch: compiled out of their kernels)
    bool hier = !SELF && npairs > 64 && G >= 1 && G * NO <= 64 && G * NS <= 64;
    if (hier) broad_quads(c, G, om, sm, neff);
    for (int base = 0; base < neff; base += 64) {
#ifdef HA_PROFILE
        unsigned long long _b0 = __builtin_amdgcn_s_memtime();
#endif
        // parallel broad phase: one pair per lane (p: its index in the flat enumeration)
        bool cand = false;
        int p = base + lane;
        int kind = -1, A = -1, B = -1;
        if (p < neff && (hier ? pair_compact(c, G, om, sm, p, kind, A, B) : pair_desc(c, p, kind, A, B))) {
            float mg = c.p->contact_margin;
            if (kind <= 3) {
                cand = c.o[A].coll != 0;
                if (kind == 2) cand = cand && c.o[B].coll != 0;
                if (cand) {
                    // an object's bounding sphere covers all its convex pieces (ha_model_t v8)
                    int pa = c.o[A].pool;
                    PoseF Po = object_pose(c, A);
                    f3 co = Po.p + qrot(Po.q, scale3(c, A, ld3(m.pool_center[pa])));
                    float ro = scale_radius(c, A, m.pool_radius[pa]);
                    if (kind == 0) {
                        cand = co.z - ro <= mg;
                    } else {
                        PoseF Pb;
                        f3 cl;
                        float rb;
                        if (kind == 1) {
                            int hb = m.static_hull[B];
                            Pb = static_pose(c, B); cl = ld3(m.hull_center[hb]); rb = m.hull_radius[hb];
                        } else if (kind == 2) {
                            int pb = c.o[B].pool;
                            Pb = object_pose(c, B); cl = ld3(m.pool_center[pb]); rb = m.pool_radius[pb];
                        } else {
                            int Lk = m.hull_link[B];
                            Pb = PoseF{ld3(s.lp[Lk]), ldq(s.lq[Lk])}; cl = ld3(m.hull_center[B]); rb = m.hull_radius[B];
                        }
                        int bb = kind == 2 ? B : -1;
                        f3 cbb = Pb.p + qrot(Pb.q, scale3(c, bb, cl));
                        f3 dc = co - cbb;
                        float rr = ro + scale_radius(c, bb, rb) + mg;
                        cand = dot3(dc, dc) <= rr * rr;
                        if (kind == 1) cand = cand && sphere_near_box(m.static_half[B], Pb, co, ro + mg);
                    }
                }
            } else {
                int Lk = m.hull_link[A];
                cand = m.link_table_collide[Lk] != 0;
                if (cand) {
                    PoseF Pst = static_pose(c, B);
                    int hs = m.static_hull[B];
                    f3 ch = ld3(s.lp[Lk]) + qrot(ldq(s.lq[Lk]), ld3(m.hull_center[A]));
                    f3 ct = Pst.p + qrot(Pst.q, ld3(m.hull_center[hs]));
                    f3 dc = ch - ct;
                    float rr = m.hull_radius[A] + m.hull_radius[hs] + mg;
                    cand = dot3(dc, dc) <= rr * rr;
                    // a table's bounding sphere (0.71 m) contains the whole hand: cull on the exact box
                    cand = cand && sphere_near_box(m.static_half[B], Pst, ch, m.hull_radius[A] + mg);
                }
            }
        }
        uint64_t mask = __ballot(cand);
#ifndef HA_X_NO_BOX_CULL     /* A/B timing builds only: the broad phase without its box cull */
        // the box cull of the candidates (pair_boxes_near), in a block of its own that derives everything from the pair
        // index again, so that none of its values stay live into the narrow phases (VGPRs). The Allegro families only
        // (SELF): A/B on one box, C3 4.94 -> 4.71 ms, C2 1.010 -> 0.975 ms; C4 +1%, C5 +0.5% (their link hulls seldom
        // come near an object, and the cull's registers cost the Ur5Sih kernels spills)
        if (SELF && mask) {
            bool keep = false;
            if ((mask >> lane) & 1ull) {
                int kd, a_, b_;
                pair_desc(c, p, kd, a_, b_);
                keep = kd == 0 || pair_boxes_near(c, kd, a_, b_, c.p->contact_margin);
            }
            mask = __ballot(keep);
            asm volatile("" : "+s"(mask));
            cand = (mask >> lane) & 1ull;
        }
#endif
        // the candidates whose persistent-manifold record applies (ha_params_t v13), tested for the whole batch at once;
        // each record is loaded at its turn (loading it one refresh ahead measured C4 +1.5%, C5 -0.7%, C2 / C4w +-0:
        // profiles/r06_ab_record_prefetch.txt)
        uint64_t vmask = __ballot(c.pcm && cand && pcm_valid_lane(c, p, kind, A, B));
        // and the candidates' separating-face records, one byte load each
        int frec = (cand && c.pairf) ? (int)c.pairf[p] : 0xFF;
#ifdef HA_PROFILE
        {   // the batch's broad phase: sphere / box tests, record validity, face-record loads (waited for here)
            int fw = wave_min_i(frec);
            wsync();
            PROF_COUNT(93, __builtin_amdgcn_s_memtime() - _b0 + (fw < -1 ? 1 : 0));
            PROF_COUNT(94, 1);
        }
#endif
        // one iteration per piece pair: a compound object (several convex pieces, ha_model_t v8) runs piece
        // pairs j = 0 .. np-1 of a candidate pair and then emits a single <= 4-point manifold for the object pair
        // (the oracle's gather_begin / gather_end). One loop and one call site per narrow phase (a single inlined
        // copy; a nested piece loop would keep its hoisted invariants live over the narrow phase: VGPRs)
        int j = 0;
        uint64_t pmask = 0;
        while (mask) {
            int bit = __ffsll((unsigned long long)mask) - 1;
            int q = base + bit;
            if (hier) pair_compact(c, G, om, sm, q, kind, A, B);
            else pair_desc(c, q, kind, A, B);
            // the pair is wave-uniform: say so, so that the narrow phase branches on scalars (no exec-masked regions)
            kind = __builtin_amdgcn_readfirstlane(kind);
            A = __builtin_amdgcn_readfirstlane(A);
            B = __builtin_amdgcn_readfirstlane(B);
#ifdef HA_PROFILE
            c.pk = kind;
#endif
            if (j == 0 && c.pcm) {
                // the pair's persistent manifold: refreshed from its record, or the narrow phase writes the record
                c.pslot = -1;
                if ((vmask >> bit) & 1ull) {
#ifdef HA_PROFILE
                    unsigned long long _r0 = __builtin_amdgcn_s_memtime();
#endif
                    pcm_emit_record(c, pcm_load(c, q), kind, A, B);
#ifdef HA_PROFILE
                    wsync();
                    PROF_COUNT(88, __builtin_amdgcn_s_memtime() - _r0);     // refreshes
                    PROF_COUNT(89, 1);
#endif
                    mask &= mask - 1;
                    continue;
                }
                c.pslot = q; c.pkind = kind; c.pA = A; c.pB = B;
            }
            int np = pair_pieces(c, kind, A, B);
            int rec = 0xFF;
            if (c.pairf && kind != 0 && np == 1) {
                rec = __builtin_amdgcn_readlane(frec, bit);
#ifdef HA_PROFILE
                unsigned long long _f0 = __builtin_amdgcn_s_memtime();
#endif
                bool fskip = rec != 0xFF && sep_face_skip(c, kind, A, B, rec);
#ifdef HA_PROFILE
                if (rec != 0xFF) {
                    wsync();
                    PROF_COUNT(90, __builtin_amdgcn_s_memtime() - _f0);     // face-record checks: time / checks / skips
                    PROF_COUNT(91, 1);
                    PROF_COUNT(92, fskip);
                }
#endif
                if (fskip) {
                    c.pslot = -1;
                    mask &= mask - 1;
                    continue;                    // separated on that face, as the narrow phase would find
                }
            }
#ifdef HA_PROFILE
            unsigned long long _k0 = __builtin_amdgcn_s_memtime();
            int _nc0 = s.nc;
#endif
            if (np > 1 && j == 0) {
                if (lane == 0) s.ng = 0;
                c.gather = true;
                wsync();
            }
            // a compound pair's piece pairs that can touch (piece_mask, 64 at a time); the others run no narrow phase
            bool run = true;
            if constexpr (!SELF) {
                if (np > 1 && (kind == 2 || kind == 3)) {
                    if ((j & 63) == 0) pmask = piece_mask(c, kind, A, B, j, np);
                    uint64_t rest = pmask >> (j & 63);
                    run = (rest & 1ull) != 0;
                    if (!run) {
                        // straight to the next piece pair that can touch (or the chunk's end): the loop's ++j lands there
                        rest >>= 1;
                        int nxt = rest ? j + __ffsll((unsigned long long)rest) : (j | 63) + 1;
                        j = (nxt < np ? nxt : np) - 1;
                    }
                }
            }
#ifdef HA_AB_NARROW_TWICE
            for (int rep = 0; rep < 2 && run; rep++) {     // one call site: the same code size as the product
                if (rep == 1) { c.dry = true; c.colA_h = c.colB_h = -1; }
                narrow_phase(c, kind, A, B, j);
            }
            c.dry = false;
#else
            if (run) narrow_phase(c, kind, A, B, j);
#endif
            if (++j < np) continue;
            j = 0;
            mask &= mask - 1;
            if (np > 1) {
                c.gather = false;
                gather_emit(c, kind, A, B);
            }
            pcm_commit(c);
            c.pslot = -1;
            if (c.pairf && kind != 0 && np == 1 && lane == 0 && c.sepf != rec) c.pairf[q] = (uint8_t)c.sepf;
#ifdef HA_PROFILE
            wsync();
            PROF_COUNT(10 + kind, __builtin_amdgcn_s_memtime() - _k0);     // time / pairs / pairs with contacts
            PROF_COUNT(15 + kind, 1);
            PROF_COUNT(20 + kind, s.nc != _nc0);
#endif
        }
    }
    wsync();
    if constexpr (SELF) detect_self(c, npairs);
}
