// ha_family.h - the kernel families: one per task, plus the Ur5Sih clutter family (bin-picking, BASELINE config 5: up to
// 8 objects, two contact chunks, a 65-coordinate velocity) that runs the same Ur5Sih task math. ha_create picks the
// family from the task and the object count.
//
// Family<FAM> is the one place a family is described: every per-family constant is a member here, the kernels
// (handarm_hip.hip env_body / contacts_body) read the members, and the host's FamilyInfo table is filled from them. To
// add a family or a per-family limit, edit Family<FAM> and nothing else. The -D overridable defaults sit beside the
// members they govern, with the measurements behind each value.
#pragma once
#include "ha_physics.h"
#include "ah_task.h"
#include "ak_task.h"

#define FAM_UR5SIH_CLUTTER 3

// the broad phase's pairs (detect's enumeration: per object its ground, statics, later objects and link hulls; then link
// hulls x statics). The Allegro families' self pairs follow them where a count includes them (the persistent-manifold
// record slots)
__host__ __device__ inline size_t pair_slots(int NO, int NS, int NLH) {
    return (size_t)NO * (1 + NS + NLH) + (size_t)(NO * (NO - 1) / 2) + (size_t)NLH * NS;
}

template <int FAM>
struct Family {
    static_assert(FAM == HA_TASK_UR5SIH || FAM == FAM_UR5SIH_CLUTTER || FAM == HA_TASK_ALLEGRO_HAND ||
                      FAM == HA_TASK_ALLEGRO_KUKA, "unknown kernel family");
    // a member's value: one per family, in this order
    template <class T>
    static constexpr T pick(T ur5sih, T clutter, T allegro_hand, T allegro_kuka) {
        return FAM == HA_TASK_UR5SIH ? ur5sih
               : (FAM == FAM_UR5SIH_CLUTTER ? clutter : (FAM == HA_TASK_ALLEGRO_HAND ? allegro_hand : allegro_kuka));
    }

    static constexpr int task = pick(HA_TASK_UR5SIH, HA_TASK_UR5SIH, HA_TASK_ALLEGRO_HAND, HA_TASK_ALLEGRO_KUKA);
    // the kernels are compiled for the task's DOF count (register-resident factorization)
    static constexpr int nd = pick(HA_ND, HA_ND, AH_ND, AK_ND);
    // object slots in LDS per env (objects per env the family's kernels support)
    static constexpr int obj_capacity = pick(3, HA_MAX_OBJ, 1, 1);

// contact chunks (MAXC contacts each). The clutter family holds 84 contacts per substep: a settled 8-object bin
// offers 59 on average and at most ~90 (bench contact_stats), 42 were at capacity in 99% of substeps.
#ifndef HB_CHUNKS
#define HB_CHUNKS 4
#endif
// Ur5Sih (3 objects) and AllegroHand: overflow chunks (PhysCfg OVF). Chunk 0 keeps the one-chunk LDS layout (21 /
// 12 contacts); the further chunks' contact entries, rows and row constants live in the env's global area, touched
// only by substeps with more contacts than chunk 0 holds. Round 3 measured C4 over 21 contacts in 5.4% of the
// substeps of a whole episode (per-env maximum 57 at p99) and C3 over 12 in 3.2% (maximum 41)
#ifndef HA_CHUNKS
#define HA_CHUNKS 4
#endif
#ifndef HA_AH_CHUNKS
#define HA_AH_CHUNKS 4
#endif
// AllegroKuka: with the hand's self-collision (v12) a substep offers 12 contacts on average and up to ~50 under random
// actions; chunk 0 holds 21 in LDS, a second chunk in the env's global area takes the rest
#ifndef HA_AK_CHUNKS
#define HA_AK_CHUNKS 2
#endif
    static constexpr int contact_chunks = pick(HA_CHUNKS, HB_CHUNKS, HA_AH_CHUNKS, HA_AK_CHUNKS);
    // every family but the clutter family keeps the chunks past chunk 0 in the env's global area (PhysCfg OVF)
    static constexpr bool overflow = pick(true, false, true, true);

// clutter chunks whose object-block rows stay in LDS (0..4); the rest go to the env's global row area, which the
// PGS reads one contact ahead. 0: env block 16.8 KB, 9 workgroups per CU (1: 22.0 KB, 7 per CU): C5 shard
// 23.0 -> 19.5 ms (tools/ab_variants.sh binpick)
#ifndef HB_LDS_CHUNKS
#define HB_LDS_CHUNKS 0
#endif
    static constexpr int lds_chunks = pick(contact_chunks, HB_LDS_CHUNKS, contact_chunks, contact_chunks);

// AllegroKuka / AllegroHand (one dense chunk): contacts per substep, and waves per SIMD asked of their
// register allocation. 12 contacts put the env block at 13.6 KB of LDS and 3 waves per SIMD cap the kernels at
// 168 VGPRs (84 / 72 B/lane scratch), so 12 workgroups run per CU instead of 8 (LDS 20.1 / 16.6 KB, 193
// VGPRs): C2 0.705 -> 0.652 ms, C3 3.23 -> 2.70 ms (tools/ab_variants.sh). The list is then over capacity in
// 1.3% (C2) / 2.0% (C3) of substeps, where the shallowest contacts give way (bench contact_stats).
// AllegroKuka holds a full chunk (21) since round 3: with 2 LDS link slots its rows still fit in front of S in the
// phase union (9.3 KB env block, 16 workgroups per CU); C2 over capacity 1.3% -> 0.09% of substeps for +2.7%
// step time. AllegroHand stays at 12: 21 in the compact layout cost +9% (0.12%), the dense rows do not fit.
// Waves per SIMD: AllegroKuka asks for 3 since round 5 (168 VGPRs, 8 B/lane scratch): with the self pass and the
// persistent manifolds it needed 120 B/lane of spills at 4, whose scratch write-backs were 43% of its HBM traffic
// (48.8 -> 27.8 KB per env) and cost more than the fourth wave won (C2 kernel 1.064 -> 1.043 ms,
// tools/diag/ab_traffic.sh); AllegroHand stays at 4 (16384 envs: the fourth wave per SIMD is worth 10% there).
#ifndef HA_AK_CONTACTS
#define HA_AK_CONTACTS 21
#endif
#ifndef HA_AH_CONTACTS
#define HA_AH_CONTACTS 12
#endif
#ifndef HA_AK_WAVES_PER_EU
#define HA_AK_WAVES_PER_EU 3
#endif
#ifndef HA_AH_WAVES_PER_EU
#define HA_AH_WAVES_PER_EU 4
#endif
    static constexpr int chunk_capacity = pick(MAXC, MAXC, HA_AH_CONTACTS, HA_AK_CONTACTS);
// minimum waves per SIMD asked of the Ur5Sih (3-object) kernels' register allocation: 3 (<= 168 VGPRs; 149
// without spills now) so the VGPRs allow the 12 workgroups per CU the LDS does
#ifndef HA_WAVES_PER_EU
#define HA_WAVES_PER_EU 3
#endif
#ifndef HB_WAVES_PER_EU
#define HB_WAVES_PER_EU 3
#endif
    static constexpr int waves_per_eu = pick(HA_WAVES_PER_EU, HB_WAVES_PER_EU, HA_AH_WAVES_PER_EU, HA_AK_WAVES_PER_EU);

    // largest hull a family's narrow-phase scratch holds: the YCB pool hulls have up to 64 vertices and 124 face
    // planes; the Allegro scenes' hulls (cooked to <= 32 vertices, <= 60 planes) take half, which puts the
    // AllegroHand env block at 10.2 KB: 16 workgroups per CU with 4 waves per SIMD
    static constexpr int col_verts = pick(64, 64, 32, 32);
    static constexpr int col_planes = pick(124, 124, 64, 64);

// AllegroKuka env block (PhysCfg SPLIT / NG / MU): split rows with HA_AK_LINK_SLOTS link contacts in LDS, no
// compound-object gather buffer (its one object is a cuboid; ha_create enforces one hull per pool object) and
// S ~ M^-1 inside the phase union: 13.3 -> 9.1 KB, so 16 workgroups per CU hold the 4096 envs of config C2 in
// one round (12 per CU ran them in 1.33 rounds). HA_AK_COMPACT=0 restores the round-2 layout (A/B timing).
#ifndef HA_AK_COMPACT
#define HA_AK_COMPACT 1
#endif
// AllegroHand in the same compact layout (split rows, no gather buffer, S in the union): every AllegroHand contact
// touches a finger link, so its rows are robot blocks in HA_AH_LINK_SLOTS LDS slots and the global spill rows
#ifndef HA_AH_COMPACT
#define HA_AH_COMPACT 0
#endif
    static constexpr bool compact = pick(false, false, HA_AH_COMPACT != 0, HA_AK_COMPACT != 0);

// clutter family: link contacts whose robot blocks stay in LDS (the rest use the global spill rows). 2 slots
// keep the env block at <= 20 KB, i.e. 8 workgroups per CU (8 slots: 22.8 KB, 7 per CU)
#ifndef HB_LINK_SLOTS
#define HB_LINK_SLOTS 2
#endif
// the Ur5Sih 3-object family's LDS link slots (split rows, HA_SPLIT_ABOVE_OCAP): 4 put the env block at 13.5 KB,
// 12 workgroups per CU (8 slots: 15.1 KB, 10 per CU): C4 shard 5.24 -> 5.01 ms; more link contacts use the
// global spill rows (tests/test_gpu_parity.py::test_link_contacts_spill_rows_match_oracle)
#ifndef HA_LINK_SLOTS
#define HA_LINK_SLOTS 4
#endif
// the compact layout's link slots, AllegroKuka
// (3 in round 4: with the hand's self contacts most contacts touch links. 9 since round 5: at 3 waves per SIMD the
// CU holds 12 workgroups, so the LDS may grow to 13.3 KB per env (552 B per slot; 9 is the most that keeps 12 per CU).
// A/B on C2 (profiles/README.md): 3 slots 1.037 ms / 27.8 KB HBM per env, 6 slots 1.018 ms / 20.5 KB, 9 slots
// 1.015 ms / 14.5 KB)
#ifndef HA_AK_LINK_SLOTS
#define HA_AK_LINK_SLOTS 9
#endif
#ifndef HA_AH_LINK_SLOTS
#define HA_AH_LINK_SLOTS 5
#endif
    static constexpr int link_slots = pick(HA_LINK_SLOTS, HB_LINK_SLOTS, compact ? HA_AH_LINK_SLOTS : HA_LINK_SLOTS,
                                           compact ? HA_AK_LINK_SLOTS : HA_LINK_SLOTS);

    // persistent contact manifolds (v13) are compiled into every family but AllegroHand: with them its kernel needs 76 B/lane
    // of register spills (44 without) and measured 4.8 -> 5.0 ms per C3 step with twice the HBM traffic; its hand closes on
    // the cube and on itself every step, so few of its pairs keep a record long enough to pay back
    static constexpr bool pcm = pick(true, true, false, true);
    // self-collision pairs (v12): only the Allegro families' kernels run them, so only their models may carry them
    static constexpr bool selfc = pick(false, false, true, true);
#ifdef HA_X_NO_SELF     /* A/B timing builds only: the Allegro families without their self-collision pass */
    static constexpr bool self_pass = false;
#else
    static constexpr bool self_pass = selfc;
#endif

// clutter family: the contacts that touch no robot link are solved in packed passes (four contacts on disjoint objects
// per pass, one per 16-lane row) instead of one whole-wave contact block after another (PhysCfg PACK);
// the oracle follows the same order for the configurations this family runs (physics_oracle.c packed_pgs)
#ifndef HB_PACKED_PGS
#define HB_PACKED_PGS 1
#endif
// the Ur5Sih 3-object family can pack the substeps whose contacts fit chunk 0 (<= 21: rows in LDS, the constants per
// contact in PK, the rest serial over the overflow chunks): measured off. Three objects give passes of at most three
// contacts, a bench env offers ~12 of which ~4 objects' worth share an object, so a sweep still runs ~4-5 passes of
// ~2-3 contacts, each slower than the serial block it replaces: C4 shard 3.14 -> 3.60 ms per step (r5j-r5p,
// bit-identical; with lane-permuted constants 3.69 ms). A -DHA_PACKED_PGS=1 build needs the oracle's h->packed = 1
#ifndef HA_PACKED_PGS
#define HA_PACKED_PGS 0
#endif
    static constexpr bool packed_pgs = pick(HA_PACKED_PGS != 0, HB_PACKED_PGS != 0, false, false);

// clutter family: 1 recomputes the object blocks of the contact rows in registers from the contact entries in the
// rows phase and at every PGS fetch (PhysCfg RC) instead of storing them in the env's global row area. Measured on
// C5 (round 3): 22.1 -> 30.8 ms per step, the ~140 VALU per fetch cost more than the stored rows' traffic, which the
// one-contact-ahead prefetch hides; the product keeps the stored rows
#ifndef HB_RECOMPUTE
#define HB_RECOMPUTE 0
#endif
    static constexpr bool recompute = pick(false, HB_RECOMPUTE != 0, false, false);

    // separating-face records of the broad phase's pairs: the clutter family only. There most candidate object pairs in
    // the bin are apart (5.8 narrow phases a substep, 0.2 with contacts) and each needs a fresh hull setup; with the
    // records 4.8 of them are skipped (narrow phases 13.8% -> 2.2% of the substep, checks 5.9%). In the Allegro
    // families the separated pairs are link hulls against the cube, whose side is cached across consecutive pairs so
    // the narrow phase's sphere cull is cheaper than a record check (C3: checks 6.8% for 3.5% saved), and the record
    // register cost spills (tools/phase_profile.py, r5l)
    static constexpr bool pair_face_records = pick(false, true, false, false);

    // the rows phase's diagonal term J_r . Y_r from Y_r read back in one batch after the loop over the DOFs (ha_solve.h
    // substep YBATCH) instead of one reload of J_r[i] per DOF behind each store of Y_r[i]. Not AllegroHand: at 4 waves
    // per SIMD (128 VGPRs) the second 22-float array costs its kernels scratch (ah_step_kernel 100 -> 120 B/lane,
    // ah_simulate_kernel 92 -> 104; tools/res_usage.sh). Not the clutter family: no resource moves, but C5 measured
    // 0.4% slower with it and level without (profiles/r10_rows_round_trips.txt). Both keep the reload
    static constexpr bool rows_y_batch = pick(true, false, false, true);

    // the physics' compile-time shape (ha_physics.h). The compact layout: split rows, no gather buffer, S in the union
    using Phys = PhysCfg<nd, obj_capacity, contact_chunks, link_slots, lds_chunks, chunk_capacity, col_verts, col_planes,
                         compact ? 1 : -1, compact ? 0 : HA_MAX_GATHER, compact, recompute, overflow, self_pass,
                         packed_pgs>;
};
template <int FAM>
using FamPhys = typename Family<FAM>::Phys;
