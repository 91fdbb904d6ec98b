"""C-ABI boundary checks that need no GPU: the library loads, exports every declared symbol, and
the ctypes mirrors of the structs match the compiled layouts (HIP library and C oracle)."""
import ctypes as C

import pytest

from handarm_hip import _lib
from handarm_hip import model as HM


@pytest.fixture(scope="module")
def lib():
    from handarm_hip import build
    build.build()
    return _lib.load()


def test_exports_every_declared_symbol(lib):
    names = _lib.header_symbols()
    assert len(names) >= 17
    for n in names:
        assert hasattr(lib, n), n
    assert set(names) == set(_lib.SIGNATURES), "ctypes signature table out of sync with include/handarm_abi.h"


def test_struct_layouts_match(lib):
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.ha_struct_sizes(C.byref(a), C.byref(b), C.byref(c)) == 0
    assert (a.value, b.value, c.value) == (C.sizeof(HM.HaModel), C.sizeof(HM.HaParams), C.sizeof(HM.HaState))
    assert lib.ha_abi_version() == 16


def test_oracle_struct_layouts_match():
    from oracle import oracle_lib
    ol = oracle_lib.load()
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    ol.hao_struct_sizes(C.byref(a), C.byref(b), C.byref(c))
    assert (a.value, b.value, c.value) == (C.sizeof(HM.HaModel), C.sizeof(HM.HaParams), C.sizeof(HM.HaState))


def test_create_rejects_bad_arguments(lib):
    m = HM.build_model(HM.load_scene())
    p, _ = HM.build_params()
    h = C.c_void_p()
    assert lib.ha_create(C.byref(m), C.byref(p), 0, C.byref(h)) == -1        # HA_E_ARG, no GPU touched
    p.num_initial_poses = 0
    assert lib.ha_create(C.byref(m), C.byref(p), 4, C.byref(h)) == -1
    assert lib.ha_simulate(None, 1, 0, None) != 0
    assert lib.ha_task_step(None, 0, None) != 0


# ha_create's refusals, one perturbed field per case. Every case starts from a scene's own model and the task's own
# params and returns before the first HIP call, so it runs without a GPU. Limits are mirrored from the kernel families
# (csrc/ha_family.h, ha_physics.h PhysCfg / ColLayout): the test pins the codes, not the table.
E_ARG, E_MODEL = -1, -4
PAIRF_LINK_HULLS = 64                                   # HA_PAIRF_LINK_HULLS
BASES = {      # asset, task, task_cfg, object slots of the family, (hull vertices, planes, gather points) of its scratch
    "ur5sih": (HM.ASSET, HM.TASK_UR5SIH, None, 3, (64, 124, 32)),
    "bin": (HM.BIN_ASSET, HM.TASK_UR5SIH, {"n_objects": 8}, 8, (64, 124, 32)),
    "allegro_hand": (HM.ALLEGRO_ASSET, HM.TASK_ALLEGRO_HAND, None, 1, (32, 64, 32)),
    "allegro_kuka": (HM.KUKA_ASSET, HM.TASK_ALLEGRO_KUKA, None, 1, (32, 64, 0)),
}
_BASE_CACHE = {}


def _base(name):
    """Fresh copies of the base's model and params (the cached originals stay unchanged)."""
    if name not in _BASE_CACHE:
        asset, task, cfg, _, _ = BASES[name]
        _BASE_CACHE[name] = (HM.build_model(HM.load_scene(asset)), HM.build_params(cfg, task=task)[0])
    m, p = _BASE_CACHE[name]
    return HM.HaModel.from_buffer_copy(m), HM.HaParams.from_buffer_copy(p)


def _col_bytes(name):
    cv, cp, ng = BASES[name][4]                         # ColLayout<CV, CP, NG>::bytes
    return 2 * 16 * cv + 2 * 16 * cp + 2 * 4 * cv + 2 * 16 * ng


def _pairf_bytes(name):
    ocap = BASES[name][3]                               # PhysCfg::pairf_bytes
    return ocap * (1 + HM.MAX_STATIC + ocap + PAIRF_LINK_HULLS) + PAIRF_LINK_HULLS * HM.MAX_STATIC


def _pairs(NO, NS, NLH):
    return NO * (1 + NS + NLH) + NO * (NO - 1) // 2 + NLH * NS       # the broad phase's pairs (ha_create)


def _box_hull(m, k):
    """Give hull k the box the broad phase's cull asks of a link hull or a compound object's piece."""
    import numpy as np
    v0, nv = m.hull_vert_start[k], m.hull_nverts[k]
    m.hull_obb[k][:] = HM.hull_obb(np.ctypeslib.as_array(m.verts)[v0:v0 + nv, :3])


def _grow_link_hulls(m, n):
    """n link hulls that pass every per-hull check: the hulls behind the scene's link hulls get a box of their own (a
    one-piece object's hull has one), further hulls are copies of hull 0."""
    pool = {m.pool_hull[i] for i in range(m.n_pool) if m.pool_nhull[i] == 1}
    for k in range(m.n_link_hulls, n):
        if k >= m.n_hulls:
            for f in ("hull_link", "hull_vert_start", "hull_nverts", "hull_plane_start", "hull_nplanes", "hull_radius",
                      "hull_edge_start", "hull_nedges"):
                getattr(m, f)[k] = getattr(m, f)[0]
            m.hull_center[k][:] = m.hull_center[0][:]
            m.hull_obb[k][:] = m.hull_obb[0][:]
        elif k not in pool:
            _box_hull(m, k)
    m.n_hulls = max(m.n_hulls, n)
    m.n_link_hulls = n


def _min_link_hulls_over_scratch(name, m):
    """Smallest n_link_hulls whose self-pair pass no longer fits the family's narrow-phase scratch (ha_create: a 64-byte
    box per link hull, 2 bytes per pair, 64 candidate entries)."""
    n = m.n_link_hulls
    while n * 64 + 2 * m.n_self_pairs + 128 <= _col_bytes(name):
        n += 1
    return n


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)


def _hull_size(field, n):
    def f(name, m, p):
        getattr(m, field)[0] = n
    return f


def _clutter(n_objects):
    def f(name, m, p):
        _set(p, n_objects=n_objects, num_obs=HM.ur5sih_num_obs(n_objects))
        if n_objects > 8:           # room for the ninth object's actor and body, so the capacity check is the one that refuses
            _set(m, n_actors=m.actor_object0 + n_objects, n_bodies=m.body_object0 + n_objects)
    return f


def _self_pair_on_ur5sih(name, m, p):
    m.n_self_pairs = 1
    m.self_pair[0] = 0 | (1 << 8)


def _self_scratch(over):
    def f(name, m, p):
        _grow_link_hulls(m, _min_link_hulls_over_scratch(name, m) - (0 if over else 1))
    return f


def _pairf(over):
    def f(name, m, p):
        # the most statics and no self pairs (their scratch check comes first), then the smallest n_link_hulls over
        _set(m, n_static=HM.MAX_STATIC, n_self_pairs=0)
        n = m.n_link_hulls
        while _pairs(p.n_objects, m.n_static, n) <= _pairf_bytes(name):
            n += 1
        _grow_link_hulls(m, n if over else n - 1)
    return f


def _multi_hull_pool_object(name, m, p):
    m.pool_nhull[0] = 2             # the cuboid and the hull behind it (the table's), boxed like a compound's pieces
    _box_hull(m, m.pool_hull[0] + 1)


_none = lambda name, m, p: None         # noqa: E731
# (id, base, perturbation, code with valid params, code with num_initial_poses = 0). ha_create checks num_initial_poses
# after the whole model, so E_ARG in the last column shows that the model passed every model check: the bases do, and so
# do the at-the-limit twins of the cases that compute a smallest violating size.
REFUSALS = [
    ("ur5sih_base", "ur5sih", _none, None, E_ARG),
    ("bin_base", "bin", _none, None, E_ARG),
    ("allegro_hand_base", "allegro_hand", _none, None, E_ARG),
    ("allegro_kuka_base", "allegro_kuka", _none, None, E_ARG),
    ("ur5sih_n_dofs", "ur5sih", lambda n, m, p: _set(m, n_dofs=16), E_MODEL, E_MODEL),
    ("allegro_hand_n_dofs", "allegro_hand", lambda n, m, p: _set(m, n_dofs=17), E_MODEL, E_MODEL),
    ("allegro_kuka_n_dofs", "allegro_kuka", lambda n, m, p: _set(m, n_dofs=17), E_MODEL, E_MODEL),
    ("allegro_hand_33_verts", "allegro_hand", _hull_size("hull_nverts", 33), E_MODEL, E_MODEL),
    ("allegro_hand_65_planes", "allegro_hand", _hull_size("hull_nplanes", 65), E_MODEL, E_MODEL),
    ("allegro_kuka_33_verts", "allegro_kuka", _hull_size("hull_nverts", 33), E_MODEL, E_MODEL),
    ("allegro_kuka_65_planes", "allegro_kuka", _hull_size("hull_nplanes", 65), E_MODEL, E_MODEL),
    ("ur5sih_65_verts", "ur5sih", _hull_size("hull_nverts", 65), E_MODEL, E_MODEL),
    ("ur5sih_125_planes", "ur5sih", _hull_size("hull_nplanes", 125), E_MODEL, E_MODEL),
    ("bin_65_verts", "bin", _hull_size("hull_nverts", 65), E_MODEL, E_MODEL),
    ("bin_125_planes", "bin", _hull_size("hull_nplanes", 125), E_MODEL, E_MODEL),
    ("allegro_kuka_multi_hull_object", "allegro_kuka", _multi_hull_pool_object, E_MODEL, E_MODEL),
    ("clutter_4_objects", "bin", _clutter(4), None, E_ARG),
    ("clutter_9_objects", "bin", _clutter(9), E_MODEL, E_MODEL),
    ("ur5sih_self_pairs", "ur5sih", _self_pair_on_ur5sih, E_MODEL, E_MODEL),
    ("allegro_hand_self_scratch_limit", "allegro_hand", _self_scratch(False), None, E_ARG),
    ("allegro_hand_self_scratch_over", "allegro_hand", _self_scratch(True), E_MODEL, E_MODEL),
    ("allegro_kuka_self_scratch_limit", "allegro_kuka", _self_scratch(False), None, E_ARG),
    ("allegro_kuka_self_scratch_over", "allegro_kuka", _self_scratch(True), E_MODEL, E_MODEL),
    ("allegro_hand_pairf_limit", "allegro_hand", _pairf(False), None, E_ARG),
    ("allegro_hand_pairf_over", "allegro_hand", _pairf(True), E_MODEL, E_ARG),
    ("allegro_hand_pcm", "allegro_hand", lambda n, m, p: _set(p, pcm_lin_tol=0.001), E_ARG, E_ARG),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_create_refusal_codes(lib, case):
    _, name, perturb, code, code_no_poses = case
    for poses, want in ((1, code), (0, code_no_poses)):
        if want is None:            # the call would be accepted and reach the device: the GPU tests' side
            continue
        m, p = _base(name)
        perturb(name, m, p)
        p.num_initial_poses = poses
        h = C.c_void_p()
        assert lib.ha_create(C.byref(m), C.byref(p), 4, C.byref(h)) == want
        assert not h.value          # a refusal hands out no handle


def test_no_cpu_fallback_on_cpu_device():
    from handarm_hip.sim import HandArmSim
    with pytest.raises(_lib.HandArmError):
        HandArmSim(4, device="cpu")
