// ha_physics.h - one-wavefront-per-environment articulated + rigid-body physics for gfx950.
//
// Algorithm (identical to oracle/physics_oracle.c, which is its scalar restatement):
//   FK (level-synchronous over the link tree) -> CRBA joint-space inertia + RNEA velocity-product
//   forces in world-frame spatial algebra -> Cholesky (lane i owns row i) -> triangular inverse
//   (lane j owns column j) -> explicit M^-1 = L^-T L^-1 -> convex-hull contacts (SAT + incident vertices,
//   <= 4 per pair) -> projected Gauss-Seidel in velocity form:
//     * joint rows (PD drives as impulse-bounded soft constraints, joint limits) live in lane d and need
//       no reduction (J = +-e_d, J v = v[d]);
//     * contact rows (normal + 2 friction) keep J_r and Y_r = M^-1 J_r^T in LDS; J_r . v is one DPP
//       row reduction + 4 v_readlane; the velocity update is one LDS read + FMA per lane.
//   Generalised velocity v lives one coordinate per lane for the whole solve -> symplectic Euler.
// Everything loops at run time (small code: the kernel must stay resident in the instruction cache),
// and the phase-local scratch (dynamics, collision, rows) shares one LDS union.
//
// Build switches of the step kernels (here and in handarm_hip.hip). None is set in the product build; a switch that
// restored a superseded implementation is removed once its comparison is recorded (profiles/), and
// tools/same_device_code.sh shows that a clean-up left the device code of each of these builds as it was.
//   HA_PROFILE               per-phase timers (g_prof, tools/phase_profile.py); HA_PROFILE_HEAVY: its heavy-substep class
//   HA_AB_TIMING             timing builds (tools/ab_build.sh): allows a repeated phase that emits no contacts
//   HA_AB_DYN_TWICE, HA_AB_FACTOR_TWICE, HA_AB_DETECT_TWICE, HA_AB_NARROW_TWICE, HA_AB_ROWS_TWICE, HA_AB_PGS_TWICE
//                            the phase run twice: (time with it twice) - (product time) = its cost in the real schedule
//   HA_X_NO_SELF             cost probe: the Allegro families without their self-collision pass
//   HA_X_SELF_NO_NARROW      cost probe: the self pass without its narrow phases
//   HA_X_SELF_DRY            cost probe: self narrow phases that emit no contacts
//   HA_X_NO_PIECE_BOX        cost probe: compound piece pairs culled by their spheres alone
//   HA_X_NO_BOX_CULL         cost probe: the broad phase without its box cull
//   HA_X_NO_PAIRF            cost probe: no separating-face records for the broad phase's pairs
//   HA_X_NO_PCM              cost probe: the persistent-manifold code compiled out
//   HA_DENSE_ROWS            every family on dense rows (tools/split_rows_check.py)
//   HA_SPLIT_ABOVE_OCAP, HA_EMIT_PARALLEL, HA_CHUNKS, HA_AH_CHUNKS, HB_LINK_SLOTS
//                            tunables with the product's value as default, each described where it is defined
#pragma once
#include <type_traits>

#include "ha_device.h"
#include "../../include/handarm_abi.h"
#include "../../include/ha_obb.h"

#define MAXC 21          /* contacts per chunk: 3 rows each -> 63 rows, one per lane (lane 63 idle) */
#define MAXR (3 * MAXC)
#define RS 35            /* max row stride: D + 6 * n_obj <= 35 (Ur5Sih); see row_stride<ND>() */
#define NOBJ HA_MAX_OBJ
#define MAXD 24
#define HA_ND 17         /* DOF count the kernels are compiled for (UR5 + SIH); checked by ha_create */
// compound object pair: reduced points gathered over its piece pairs (later ones dropped; the oracle's MAXGATHER)
#define HA_MAX_GATHER 32
#define MAXB 44          /* rigid bodies per env (contact-force rows): robot links + objects + statics (bin scene: 44) */
#define MAXV 72          /* generalized velocity coordinates D + 6 x objects (17 + 6 x 8 = 65 for bin-picking) */

// What the task observables read after refresh_simulation_tensors(): flange pose, fingertip states,
// dof positions, object root states (filled from FK in the fused step, or from the state tensors).
struct ObsIn {
    float flange[8];
    float tip[5][10];      // pos, quat, linvel
    float dofpos[MAXD];
    float obj[NOBJ][13];
    float pad[2];
};

struct DynScratch {
    float Ic[HA_MAX_LINKS][13];                 // composite spatial inertia (m, h, J) at world origin
    float Al[HA_MAX_LINKS][6], Fl[HA_MAX_LINKS][6];
};
// Narrow-phase scratch in the phase union, laid out per kernel family for its largest hull (NV vertices, NP face
// planes; ha_create checks the model against it): world vertices and planes of both hull sides, the clipping
// candidates and their max side-plane distances, and a compound pair's gathered points and normals
// (NG gathered points: HA_MAX_GATHER, or 0 for a family without compound objects, which ha_create enforces)
template <int NV, int NP, int NG = HA_MAX_GATHER>
struct ColLayout {
    static constexpr size_t wvA = 0, wvB = wvA + 16 * NV, wpA = wvB + 16 * NV, wpB = wpA + 16 * NP;
    static constexpr size_t cand = wpB + 16 * NP, cmax = cand + 4 * NV, gp = cmax + 4 * NV;
    static constexpr size_t gn = gp + 16 * NG, bytes = gn + 16 * NG;
};
struct ColView {
    float (*wvA)[4], (*wvB)[4];         // world vertices of both hulls
    float (*wpA)[4], (*wpB)[4];         // world face planes (n, d) of both hulls
    int* cand;                          // clipping: candidate incident vertices
    int* cmax;                          // clipping: per-candidate max plane distance (order-preserving int)
    float (*gp)[4], (*gn)[4];           // compound object pair: gathered points (x, sep) and normals
};
struct RowScratch {
    float J[MAXR * RS];
    float Y[MAXR * RS];
};
// Dynamics (M + spatial scratch) and, after the physics, the refresh / observation staging, which overlap:
// the staging and the last substep's joint / contact forces (written after each substep's PGS) are only read
// after the last substep, and the next substep's dynamics may overwrite them. The link twists Vl are written
// by the dynamics and again by the refresh (link_twists), and read by the observation staging, so they stay
// outside the overlap.
struct PostScratch {
    float Vl[HA_MAX_LINKS][6];                  // link twists (w, v at the world origin)
    union {
        struct {
            float M[MAXD * MAXD];               // M, then its Cholesky factor L (stride D)
            DynScratch dyn;
        };
        struct {
            ObsIn in;
            float obs[216];                     // Ur5Sih: 108 + 13 x objects (212 at 8 objects)
            float cforce[MAXB][3];
            float dforce[MAXD];                 // joint force of the last substep (drive + limits) / h
        };
    };
};

// One free object's state (LDS). These live after the EnvLDS block, one per object slot of the task
// (Ur5Sih 3, bin-picking 7, AllegroHand / AllegroKuka 1), so the object capacity costs only the tasks
// that use it.
struct ObjLDS {
    float oc[4], oq[4], ov[4], ow[4];   // COM position, orientation, linear / angular velocity
    float oIinv[9];                     // world inverse inertia (3x3)
    float otq[3];                       // v16: world torque for this physics call (apply_rigid_body_force_tensors)
    float osc[4];                       // per-env dimension scale of the pool hull; [3] = 1 when scaled
    float ofx[4];                       // world force on the COM for this physics call (apply_rigid_body_force)
    float om;                           // mass
    int pool, coll;                     // pool id, collision enabled
};

// One contact point (LDS, after the object slots): up to MAXC x chunks per env (task_lds_bytes).
// 32 bytes: the combined friction is not stored (contact_friction(a, b) again in the rows phase, the same
// value), and the body codes fit 16 bits
struct ContactLDS {
    float x[3], n[3];                   // world point, normal from body b to body a
    float sep;                          // separation (< 0: penetration)
    short a, b;                         // body codes: -1 static, 0..NOBJ-1 object, 100 + link
};
static_assert(sizeof(ContactLDS) == 32, "ContactLDS layout");

struct EnvLDS {
    float q[MAXD], qd[MAXD], tgt[MAXD];
    float lp[HA_MAX_LINKS][3], lq[HA_MAX_LINKS][4];
    float ax[MAXD][3], an[MAXD][3];
    float Cb[MAXD];
    float v[MAXV];
    int nc, nr, noff, ng;                       // contacts kept / rows / contacts offered this substep /
                                                // points gathered for a compound object pair
    int cst[HA_CSTAT];                          // contact_stats of this launch (see ha_state_t)
    float sb[8];                                // pose of the actor carrying posed statics (v14): p[3], pad, q[4]
    union {
        PostScratch pd;                         // (the narrow-phase scratch, ColLayout, is sized per family)
        RowScratch rows;
        float xfer[MAXR * HA_MAX_CONTACTS / MAXC];  // lane exchange outside the physics phases (controller;
                                                    // PGS impulses of every row -> contact forces). Must stay
                                                    // below the rows' RK area (static_assert in PhysCfg users)
    } u;
};

// Compact constraint rows: a contact touches at most two free objects, so a row stores the robot block (D)
// plus one 6-wide block per object slot (slot 0 = the lower object index, slot 1 = the other), instead of
// all D + 6 x n_obj coordinates. Ur5Sih (3 objects): stride 17 + 12; one-object tasks (AllegroHand 16,
// AllegroKuka 23 DOF): D + 6. Dot products over a compact row visit the nonzero terms in the same order as
// the dense row, so results are unchanged; the LDS saving is what lets these kernels run 8 workgroups per CU.
template <int ND>
__host__ __device__ constexpr int row_slots() { return ND == HA_ND ? 2 : 1; }
template <int ND>
__host__ __device__ constexpr int row_stride() { return ND + 6 * row_slots<ND>(); }
// object slots of a contact between bodies a and b (codes: -1 static, 0..NOBJ-1 object, 100+ link)
HD void contact_slots(int a, int b, int& so0, int& so1) {
    int oa = (a >= 0 && a < 100) ? a : -1, ob = (b >= 0 && b < 100) ? b : -1;
    so0 = oa < 0 ? ob : (ob < 0 ? oa : (oa < ob ? oa : ob));
    so1 = (oa >= 0 && ob >= 0) ? (oa < ob ? ob : oa) : -1;
}
// index of generalized coordinate `lane` in a compact row (-1: not touched by the contact)
HD int compact_index(int lane, int D, int so0, int so1) {
    if (lane < D) return lane;
    int t = lane - D;
    if (so0 >= 0 && t >= 6 * so0 && t < 6 * so0 + 6) return D + t - 6 * so0;
    if (so1 >= 0 && t >= 6 * so1 && t < 6 * so1 + 6) return D + 6 + t - 6 * so1;
    return -1;
}
// LDS block of one env: EnvLDS up to the phase union, the union at the task's row stride and contact
// chunks (J and Y of MAXR x chunks rows), then the object slots (ObjLDS x capacity), then the contact list
// (ContactLDS x MAXC x chunks), 16-byte aligned
__host__ __device__ inline size_t obj_lds_offset_rows(size_t rows) {
    size_t u = sizeof(PostScratch);
    if (rows > u) u = rows;
    return (offsetof(EnvLDS, u) + u + 15) & ~(size_t)15;
}

// Compile-time shape of a kernel family's physics: DOF count, object slots, contact chunks (MAXC contacts
// each) and velocity words per lane (coordinates lane and lane + 64 when D + 6 x objects > 64).
//
// Split rows (split = true): most clutter contacts touch no robot link (object-bin, object-object), and such a
// row's robot block is zero in J and in Y = M^-1 J^T. The rows then keep only their object blocks in LDS (OW =
// 6 x object slots floats each of J and Y), and the robot blocks of the contacts that do touch a link get a slot
// of their own: the first KL link contacts in LDS, the rest in a per-env global spill area (ha_create allocates
// it; L2-resident, rare). Every dot product visits the nonzero terms in the dense order and a skipped zero block
// adds exact zeros, so results are bit-identical to the dense rows. The Ur5Sih families (3 and 8 object slots)
// split by default (HA_SPLIT_ABOVE_OCAP); AllegroKuka (one object slot, SPLIT = 1) splits too: its cube-table
// contacts, most of the list, touch no link.
//
// Minv in the union (MU = true, AllegroKuka): S ~ M^-1 sits at the END of the phase union, over the dynamics
// scratch (dead once dynamics() has produced M and Cb) and clear of M (which factor_inverse reads while writing
// S), of the narrow-phase scratch (detect runs while S is live) and of the constraint rows (the rows phase and
// the PGS read S): the static_asserts below check the three. Otherwise S follows the union.
#ifndef HA_SPLIT_ABOVE_OCAP
#define HA_SPLIT_ABOVE_OCAP 2   /* families with more object slots use split rows (Ur5Sih 3 objects, clutter) */
#endif
//
// Overflow chunks (OVF = true, the Ur5Sih and AllegroHand families): chunk 0 keeps the family's LDS layout (contact
// entries, rows, the PGS row constants in registers), and chunks 1..NCH-1 keep their contact entries, constraint rows
// and row constants in the env's global area (L2-resident), so the contact capacity grows without LDS. A substep
// with <= CAP contacts never touches that area; a substep over CAP swaps every chunk's row constants through it.
#define HA_PAIRF_LINK_HULLS 64     /* link hulls the pair face records are sized for */
template <int ND, int OCAP, int NCH, int KL = 8, int LCH = NCH, int CAP = MAXC, int CV = 64, int CP = 128,
          int SPLIT = -1, int NG = HA_MAX_GATHER, bool MU = false, bool RC = false, bool OVF = false, bool SELF = false,
          bool PACK = false>
struct PhysCfg {
    static constexpr int nd = ND, ocap = OCAP, nch = NCH;
    // packed PGS passes (the clutter family): the contacts that touch no robot link are solved four at a time, one
    // per 16-lane row, in passes of contacts on disjoint objects (ha_physics.h substep, "free passes"); their
    // object-block rows must all be in the env's global row area
    static constexpr bool pack = PACK;
    // overflow families pack only the substeps whose contacts fit chunk 0 (their rows in LDS); max_passes also counts
    // the contacts whose constants PK holds
    static constexpr int max_passes = OVF ? CAP : CAP * NCH;
    // the family's robot collides with itself (ha_model_t v12 self pairs; the Allegro families). Without it the
    // self-pair pass is not compiled (its registers would count against every family)
    static constexpr bool selfc = SELF;
    static constexpr int colv = CV, colp = CP, colg = NG;   // largest hull: vertices, face planes; gather points
    static constexpr size_t col_bytes = ColLayout<CV, CP, NG>::bytes;
    // contacts per chunk (MAXC, or fewer: the rows and the LDS list shrink with it)
    static constexpr int cap = CAP;
    static constexpr bool ovf = OVF && NCH > 1;
    static constexpr int rpc = 3 * CAP;             // constraint rows per chunk
    static constexpr int vw = ND + 6 * OCAP > 64 ? 2 : 1;
#ifdef HA_DENSE_ROWS    /* diagnostic build (tools/split_rows_check.py): every family on dense rows */
    static constexpr bool split = false;
#else
    static constexpr bool split = SPLIT >= 0 ? SPLIT != 0 : OCAP > HA_SPLIT_ABOVE_OCAP;
#endif
    static constexpr int ow = 6 * row_slots<ND>();  // split rows: object-block width
    static constexpr int kl = KL;
    static constexpr bool minv_in_union = MU;
    // split rows with recomputed object blocks (RC, the clutter family): no object-block rows are stored at all; the
    // rows phase and the PGS evaluate a contact row's object blocks in registers from the contact entry (obj_blocks)
    static constexpr bool rc = RC && split;
    // split rows: the object blocks of chunks [0, lch) live in LDS, those of chunks [lch, nch) in the env's global
    // row area after the robot-block spill rows (written by the rows phase, read back by the PGS one contact ahead)
    // (OVF: chunk 0's rows in LDS, split or dense, the others in the global area)
    static constexpr int lch = ovf ? 1 : (split ? LCH : NCH);
    static constexpr int spill_robot = split ? 2 * 3 * (CAP * NCH - KL) * ND : 0;   // per env: J then Y
    static constexpr int spill_obj = split && !rc ? 2 * rpc * (NCH - lch) * ow : 0;  // per env: J then Y
    // OVF global area after those: dense rows of chunks 1.. (J then Y), the row constants of every chunk (6 x rpc x
    // NCH, the LDS RK layout), the contact entries of chunks 1.. (8 floats each)
    static constexpr int spill_dense = ovf && !split ? 2 * rpc * (NCH - 1) * row_stride<ND>() : 0;
    // PGS row constants (RK): 6 arrays of rk_stride floats (impulse, target velocity, 1/diagonal, friction, two Delassus
    // entries), each indexed by the row over all chunks. The kernel's rk() indexes with rk_stride and both RK areas (LDS
    // for the non-overflow multi-chunk family, the global area for OVF) are sized from it: one constant, so the index
    // range and the allocation cannot disagree (the first overflow build indexed with the LDS layout's 63-row MAXR
    // stride while AllegroHand's 12-contact chunks have 36 rows: DESIGN.md §3.12)
    static constexpr int rk_stride = rpc * NCH;
    static constexpr int spill_rk = ovf ? 6 * rk_stride : 0;
    static constexpr int spill_ct = ovf ? 8 * CAP * (NCH - 1) : 0;
    static constexpr int off_dense = spill_robot + spill_obj, off_rk = off_dense + spill_dense,
                         off_ct = off_rk + spill_rk;
    // self-collision families: one byte per self pair, the separating face of the pair's last narrow phase
    static constexpr int spill_selfc = SELF ? HA_MAX_SELF_PAIRS / 4 : 0;
    static constexpr int off_selfc = off_ct + spill_ct;
    // every family: one byte per candidate pair of detect's enumeration, the separating face of the pair's last narrow
    // phase (the self pairs' record, for the other pairs); bounded for up to HA_PAIRF_LINK_HULLS link hulls and
    // HA_MAX_STATIC statics (ha_create checks the model against it)
    static constexpr int pairf_bytes = OCAP * (1 + HA_MAX_STATIC + OCAP + HA_PAIRF_LINK_HULLS) + HA_PAIRF_LINK_HULLS * HA_MAX_STATIC;
    static constexpr int spill_pairf = (pairf_bytes + 3) / 4;
    static constexpr int off_pairf = off_selfc + spill_selfc;
    static constexpr int spill_floats = off_pairf + spill_pairf;
    static_assert(ND + 6 * OCAP <= MAXV, "generalized velocity exceeds MAXV");
    static_assert(!split || (KL >= 0 && KL <= CAP * NCH), "LDS link slots must not exceed the contact capacity");
    static_assert(!split || CAP * NCH <= 128, "split rows: <= 128 contacts");
    static_assert(split || CAP * NCH <= 64, "dense rows: <= 64 contacts (one ballot)");
    static_assert(lch >= 0 && lch <= NCH, "LDS row chunks");
    static_assert(CAP * NCH <= HA_MAX_CONTACTS, "contact capacity exceeds HA_MAX_CONTACTS");
    static_assert(CAP >= 1 && CAP <= MAXC, "contacts per chunk");
    static_assert(!ovf || !rc, "overflow chunks with recomputed object blocks");
    static_assert(NG == 0 || NG == HA_MAX_GATHER, "gather buffer: HA_MAX_GATHER points or none");
    static_assert(CP >= 8, "sat_planes reads plane slots 0..7 of the narrow-phase scratch");
    static_assert(!PACK || (SPLIT != 0 && OCAP > HA_SPLIT_ABOVE_OCAP && !RC && NCH > 1 && (OVF ? CAP <= 21 : LCH == 0)),
                  "packed passes: split rows; either every object-block row in the global area with RK in LDS, or "
                  "(overflow chunks) chunk 0's rows in LDS with their constants in registers");
};
// bytes of the constraint rows proper, then (several contact chunks only) the per-row PGS constants of every
// chunk (impulse, target velocity, 1/diag, friction, two Delassus entries: 6 floats x MAXR x chunks), which the
// PGS swaps into registers one chunk at a time
template <class PC>
__host__ __device__ constexpr size_t pc_rowdata_bytes() {
    return PC::split ? 2 * sizeof(float) * ((size_t)PC::rpc * PC::lch * PC::ow + 3 * (size_t)PC::kl * PC::nd)
                     : 2 * sizeof(float) * (size_t)PC::rpc * PC::lch * row_stride<PC::nd>();
}
// packed families (PhysCfg PACK) keep a packed substep's PGS constants per contact instead (PK, 12 floats: impulses
// l0 l1 l2, the normal row's target velocity, the three 1/diagonals, the friction coefficient, the Delassus entries
// a10 a20 a21, 0; the friction rows' target velocities are 0)
#define HA_PK 12
template <class PC>
__host__ __device__ constexpr size_t pc_rows_bytes() {
    return PC::pack ? pc_rowdata_bytes<PC>() + sizeof(float) * HA_PK * (size_t)PC::max_passes
                    : pc_rowdata_bytes<PC>() + (PC::nch > 1 && !PC::ovf ? 6 * sizeof(float) * (size_t)PC::rk_stride : 0);
}
template <class PC>
__host__ __device__ constexpr size_t pc_pk_offset() { return pc_rowdata_bytes<PC>(); }

// S ~ M^-1 (factor_inverse), D x D at stride D, sized for the family's DOF count: at the end of the union
// (minv_in_union) or after it
// (after the constraint rows when those reach past it: the union then grows by the difference, which the
// AllegroKuka layout spends on a third LDS link slot)
template <class PC>
__host__ __device__ constexpr size_t minv_union_offset() {
    size_t a = (sizeof(PostScratch) - (size_t)PC::nd * PC::nd * sizeof(float)) & ~(size_t)15;
    size_t r = (pc_rows_bytes<PC>() + 15) & ~(size_t)15;
    return a > r ? a : r;
}
template <class PC>
__host__ __device__ inline size_t minv_lds_offset() {
    if constexpr (PC::minv_in_union) {
        static_assert(offsetof(PostScratch, M) + (size_t)PC::nd * PC::nd * sizeof(float) <= minv_union_offset<PC>(),
                      "S must not overlap M (factor_inverse reads M while writing S)");
        static_assert(offsetof(PostScratch, dyn) <= minv_union_offset<PC>(), "S may overlap only the dynamics scratch");
        static_assert(PC::col_bytes <= minv_union_offset<PC>(), "S must not overlap the narrow-phase scratch");
        static_assert(pc_rows_bytes<PC>() <= minv_union_offset<PC>(), "S must not overlap the constraint rows");
        return offsetof(EnvLDS, u) + minv_union_offset<PC>();
    } else {
        return obj_lds_offset_rows(pc_rows_bytes<PC>() > PC::col_bytes ? pc_rows_bytes<PC>() : PC::col_bytes);
    }
}
// the family's narrow-phase scratch view into the phase union
template <class PC>
__device__ inline ColView col_view(void* u) {
    using L = ColLayout<PC::colv, PC::colp, PC::colg>;
    char* b = reinterpret_cast<char*>(u);
    ColView v;
    v.wvA = reinterpret_cast<float(*)[4]>(b + L::wvA); v.wvB = reinterpret_cast<float(*)[4]>(b + L::wvB);
    v.wpA = reinterpret_cast<float(*)[4]>(b + L::wpA); v.wpB = reinterpret_cast<float(*)[4]>(b + L::wpB);
    v.cand = reinterpret_cast<int*>(b + L::cand); v.cmax = reinterpret_cast<int*>(b + L::cmax);
    v.gp = reinterpret_cast<float(*)[4]>(b + L::gp); v.gn = reinterpret_cast<float(*)[4]>(b + L::gn);
    return v;
}
template <class PC>
__host__ __device__ inline size_t obj_lds_offset() {
    if constexpr (PC::minv_in_union) {
        size_t u = pc_rows_bytes<PC>() > PC::col_bytes ? pc_rows_bytes<PC>() : PC::col_bytes;
        size_t se = minv_union_offset<PC>() + (size_t)PC::nd * PC::nd * sizeof(float);
        return obj_lds_offset_rows(u > se ? u : se);
    }
    else
        return (minv_lds_offset<PC>() + (size_t)PC::nd * PC::nd * sizeof(float) + 15) & ~(size_t)15;
}
template <class PC>
__host__ __device__ inline size_t contact_lds_offset() {
    return obj_lds_offset<PC>() + (size_t)PC::ocap * sizeof(ObjLDS);
}
template <class PC>
__host__ __device__ inline size_t selfm_lds_offset() {
    return contact_lds_offset<PC>() + (size_t)PC::cap * (PC::ovf ? 1 : PC::nch) * sizeof(ContactLDS);
}
// the self-collision candidate bits (detect_self), a bit a pair, after the contact list: only in the families that
// collide the robot with itself, so the others' env blocks do not grow
template <typename PC>
__host__ __device__ inline size_t task_lds_bytes() {
    return selfm_lds_offset<PC>() + (PC::selfc ? HA_MAX_SELF_PAIRS / 8 : 0);
}

struct SimCtx {
    const ha_model_t* __restrict__ m;
    const ha_params_t* __restrict__ p;
    EnvLDS* s;
    ObjLDS* o;              // the env's object slots (after the EnvLDS block, see task_lds_bytes)
    ContactLDS* k;          // the env's contact list (after the object slots): entries [0, kc0)
    ContactLDS* kg;         // overflow chunks (PhysCfg OVF): entries [kc0, maxc) in the env's global area; null
                            // otherwise (a constant the compiler folds: ct_global is then false)
    int kc0;                // entries in LDS
    float* Minv;            // S ~ M^-1, D x D (after the phase union, see obj_lds_offset)
    ColView col;            // narrow-phase scratch of the family (col_view)
    int lane, D, NO, L;
    int maxc;               // contact capacity (MAXC x chunks of the kernel family)
    const float* dr;        // this env's domain-randomization row (HA_DR_*), or null when DR is off
    const float* drg;       // v16: the shard-wide randomization state (ha_state_t.dr_global, HA_DRG_*), null: DR off
    const ha_dr_replay_t* rp;   // HA_FLAG_REPLAY_DR: the replay buffers (device copy of ha_bind_dr_replay's struct);
                                // null: every DR draw from the counter hash
    float* spill;           // split rows: this env's global robot-block rows beyond the LDS slots (J, then Y)
    // narrow-phase cache: (hull, body) whose world vertices / planes are in ColScratch side A / side B. Within one
    // detect() the poses do not change, so consecutive pairs that share a side skip its setup (same values).
    int colA_h, colA_b, colB_h, colB_b;
    bool colA_p;            // side A's world planes are in ColScratch too (SAT B runs first and may exit before them)
    bool gather;            // a compound object pair's piece pairs: reduced points go to ColScratch gp / gn
    // self-collision pairs (PhysCfg SELF): the separating face the last narrow phase found (0x80 | k: face k of side B,
    // k: face k of side A, 0xFF: none), and the env's per-pair record of it in its global area (null otherwise)
    int sepf;
    uint8_t* selfc;
    uint8_t* pairf;         // the candidate pairs' separating-face records (PhysCfg off_pairf; null: off)
    uint32_t* selfm;        // LDS: this substep's self-pair candidates, a bit a pair (selfm_lds_offset; null otherwise)
    // VecTask.step's head and tail folded into the step launch (ha_task_step_io; null / unused otherwise): the caller's
    // raw actions, clamped to +-clip_act where the task reads them (act_at), and a second, clamped copy of obs
    const float* act_in;
    float* obs_out;
    float clip_act, clip_obs;
    // persistent contact manifolds (ha_params_t v13): this env's records (ha_state_t.contact_cache; null: off), and
    // the running pair's slot (-1: none) and description, whose narrow phase writes the record it emits
    float* pcm;
    int pslot, pkind, pA, pB;
    int pemit;              // points of the running pair's manifold staged for its record (pcm_commit), 0: none
    bool last;              // the launch's final substep (run_physics): the only one whose joint / contact forces
                            // (PostScratch dforce, cforce) are read, so the only one that builds them
#ifdef HA_PROFILE
    int pk;                 // profiled build: kind of the running pair
    int pcls;               // profiled build: this substep is heavy (g_prof's second set)
#endif
#ifdef HA_AB_TIMING
    bool dry;               // A/B timing builds only: a repeated phase that must not emit contacts
#endif
};

// obs_dict["obs"] = clamp(obs_buf, -clip, clip) (vec_task.py:437) next to obs_buf, when the launch asks for it
HD void obs_out_put(const SimCtx& c, size_t i, float v) {
    if (c.obs_out) c.obs_out[i] = fminf(fmaxf(v, -c.clip_obs), c.clip_obs);
}

// Contact entry ci of the list: LDS for [0, kc0), the env's global overflow entries after that (PhysCfg OVF). Read and
// written by value: a pointer that may address either LDS or global memory would be a flat pointer, so each access
// keeps its two address spaces on separate paths.
HD bool ct_global(const SimCtx& c, int ci) { return c.kg != nullptr && ci >= c.kc0; }
// The two branches address different memories on purpose; the address-space casts keep the compiler from merging
// them into one generic (flat) access through a selected pointer: a flat load waits on the vector-memory counter
// too, so one in the PGS loop (ct_ab) would also wait for the global rows prefetched for the next contact
#define HA_AS_LDS __attribute__((address_space(3)))
#define HA_AS_GLB __attribute__((address_space(1)))
HD const HA_AS_LDS ContactLDS* ct_lds(const SimCtx& c, int ci) { return (const HA_AS_LDS ContactLDS*)(c.k + ci); }
HD const HA_AS_GLB ContactLDS* ct_glb(const SimCtx& c, int ci) {
    return (const HA_AS_GLB ContactLDS*)(c.kg + (ci - c.kc0));
}
HD ContactLDS ct_get(const SimCtx& c, int ci) {
    ContactLDS r;
    if (ct_global(c, ci)) {
        const HA_AS_GLB ContactLDS* g = ct_glb(c, ci);
        r.x[0] = g->x[0]; r.x[1] = g->x[1]; r.x[2] = g->x[2];
        r.n[0] = g->n[0]; r.n[1] = g->n[1]; r.n[2] = g->n[2];
        r.sep = g->sep; r.a = g->a; r.b = g->b;
    } else {
        const HA_AS_LDS ContactLDS* l = ct_lds(c, ci);
        r.x[0] = l->x[0]; r.x[1] = l->x[1]; r.x[2] = l->x[2];
        r.n[0] = l->n[0]; r.n[1] = l->n[1]; r.n[2] = l->n[2];
        r.sep = l->sep; r.a = l->a; r.b = l->b;
    }
    return r;
}
HD float ct_sep(const SimCtx& c, int ci) {
    if (ct_global(c, ci)) return ct_glb(c, ci)->sep;
    return ct_lds(c, ci)->sep;
}
HD void ct_ab(const SimCtx& c, int ci, int& a, int& b) {
    if (ct_global(c, ci)) {
        a = ct_glb(c, ci)->a;
        b = ct_glb(c, ci)->b;
    } else {
        a = ct_lds(c, ci)->a;
        b = ct_lds(c, ci)->b;
    }
}
// typed views of a row pointer the caller knows to be LDS / global (the PGS fetch's two load paths stay apart)
HD auto lds_f(const float* p) { return (const HA_AS_LDS float*)p; }
HD auto glb_f(const float* p) { return (const HA_AS_GLB float*)p; }
template <typename Q>
HD void ct_fill(Q* q, f3 x, f3 n, float sep, int a, int b) {
    // eight dword stores: the two 16-bit body codes go as one packed word
    q[0] = x.x; q[1] = x.y; q[2] = x.z; q[3] = n.x; q[4] = n.y; q[5] = n.z; q[6] = sep;
    q[7] = __int_as_float((a & 0xFFFF) | (b << 16));
}
HD void ct_put(const SimCtx& c, int ci, f3 x, f3 n, float sep, int a, int b) {
    if (ct_global(c, ci)) ct_fill((HA_AS_GLB float*)(c.kg + (ci - c.kc0)), x, n, sep, a, b);
    else ct_fill((HA_AS_LDS float*)(c.k + ci), x, n, sep, a, b);
}

// friction of a contact body (link 100+L, object o, static -1) and of a contact (PhysX average combine)
HD float body_friction(const SimCtx& c, int b) {
    if (!c.dr || b < 0) return c.p->friction;
    return b >= 100 ? c.dr[HA_DR_LINK_FRIC + (b - 100)] : c.dr[HA_DR_OBJ_FRIC + b];
}
HD float contact_friction(const SimCtx& c, int a, int b) { return 0.5f * (body_friction(c, a) + body_friction(c, b)); }

// 64-lane sum: DPP butterfly inside each 16-lane row (xor1, xor2, half-mirror, mirror), then the four
// row sums via v_readlane. Every lane gets the same bits; the oracle emulates this exact tree.
HD float wave_sum_rows(float x) {
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, true));   // quad_perm 1,0,3,2
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, true));   // quad_perm 2,3,0,1
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x141, 0xF, 0xF, true));  // row_half_mirror
    x += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x140, 0xF, 0xF, true));  // row_mirror
    return rows_sum(x);     // (r3 + r2) + (r1 + r0) == (r0 + r1) + (r2 + r3) bitwise
}

// Diagnostic phase timers (built only into libhandarm_hip_prof.so, -DHA_PROFILE): lane 0 of every
// wave adds the s_memtime delta of each phase; read back with ha_profile_read().
#ifdef HA_PROFILE
// [32 + 8 kind + phase]: the hull-hull split per pair kind; a second set of 96 for the substeps whose narrow phases
// offered more than HA_PROFILE_HEAVY contacts (the previous substep's class for the phases before detect)
__device__ unsigned long long g_prof[2 * 96];
#ifndef HA_PROFILE_HEAVY
#define HA_PROFILE_HEAVY 24
#endif
#define PROF_BEGIN() unsigned long long _pt = __builtin_amdgcn_s_memtime();
#define PROF_COUNT(i, v)                                               \
    do {                                                               \
        if (c.lane == 0) atomicAdd(&g_prof[(i) + 96 * c.pcls], (unsigned long long)(v)); \
    } while (0)
#define PROF(i)                                                        \
    do {                                                               \
        wsync();                                                       \
        unsigned long long _n = __builtin_amdgcn_s_memtime();          \
        if (c.lane == 0) atomicAdd(&g_prof[(i) + 96 * c.pcls], _n - _pt); \
        _pt = _n;                                                      \
    } while (0)
#else
#define PROF_BEGIN()
#define PROF(i)
#define PROF_COUNT(i, v)
#endif

// three independent wave_sum_rows, interleaved step by step so the DPP read-after-write wait states of
// one chain are filled by the others (same reduction tree per value)
HD void wave_sum_rows3(float& a, float& b, float& c) {
    a += dpp_f<0xB1>(a); b += dpp_f<0xB1>(b); c += dpp_f<0xB1>(c);
    a += dpp_f<0x4E>(a); b += dpp_f<0x4E>(b); c += dpp_f<0x4E>(c);
    a += dpp_f<0x141>(a); b += dpp_f<0x141>(b); c += dpp_f<0x141>(c);
    a += dpp_f<0x140>(a); b += dpp_f<0x140>(b); c += dpp_f<0x140>(c);
    a = dpp_row_add<0x142, 0xA>(a); b = dpp_row_add<0x142, 0xA>(b); c = dpp_row_add<0x142, 0xA>(c);
    a = dpp_row_add<0x143, 0xC>(a); b = dpp_row_add<0x143, 0xC>(b); c = dpp_row_add<0x143, 0xC>(c);
    a = lane63(a); b = lane63(b); c = lane63(c);
}
// three 16-lane row sums (the first four steps of wave_sum_rows3): every lane of a row gets its row's
// ((x0+x1)+(x2+x3)) + ((x4+x5)+(x6+x7)) ... = (Q0+Q1)+(Q2+Q3), the oracle's row_dot16
HD void row_sum3(float& a, float& b, float& c) {
    a += dpp_f<0xB1>(a); b += dpp_f<0xB1>(b); c += dpp_f<0xB1>(c);
    a += dpp_f<0x4E>(a); b += dpp_f<0x4E>(b); c += dpp_f<0x4E>(c);
    a += dpp_f<0x141>(a); b += dpp_f<0x141>(b); c += dpp_f<0x141>(c);
    a += dpp_f<0x140>(a); b += dpp_f<0x140>(b); c += dpp_f<0x140>(c);
}

// The rest, in this order: each part uses the ones before it
#include "ha_dynamics.h"
#include "ha_collide.h"
#include "ha_solve.h"
