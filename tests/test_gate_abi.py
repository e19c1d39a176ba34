"""CPU-side checks of the pyramid gate's entry points (include/mgagate.h) on the built library: the Philox restatement of tests/philox_ref.py
against Random123's known answers and against the library's host helpers (the same inline function the kernels compile), every argument
error -- each returned before anything is launched (there is no GPU here) -- and the plans' unchanged argument lists.  The header against
the binding is tests/test_abi_headers.py's."""
import ctypes as C
import inspect

import pytest

import philox_ref as PR
from abi_header import FAKE as P

U32 = C.c_uint32


def test_restatement_reproduces_the_known_answers():
    for ctr, key, want in PR.KNOWN_ANSWERS:
        assert PR.philox4x32(ctr, key) == want
    # the vectorised form is the scalar one
    u1, u2 = PR.uniform_arrays(2 ** 40 + 7, 2 ** 32, 2, 300)
    for i in (0, 1, 255, 256, 299):
        k1, k2 = PR.uniforms(2 ** 40 + 7, 2 ** 32, 2, i)
        assert float(u1[i]) == k1 * 2.0 ** -24 and float(u2[i]) == k2 * 2.0 ** -24


def test_library_philox_gives_the_known_answers(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for ctr, key, want in PR.KNOWN_ANSWERS:
        out = (U32 * 4)()
        lib.mgagate_philox4x32((U32 * 4)(*ctr), (U32 * 2)(*key), out)
        assert tuple(out) == want, [hex(v) for v in out]


@pytest.mark.parametrize("seed", [0, 2 ** 40 + 7])
@pytest.mark.parametrize("step", [0, 1, 2 ** 32])
@pytest.mark.parametrize("stream_id", [0, 2])
def test_library_uniforms_equal_the_restatement(built_lib, seed, step, stream_id):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for i in (0, 1, 255, 256, 2 ** 24):
        out = (C.c_float * 2)()
        lib.mgagate_uniforms(seed, step, stream_id, i, out)
        k1, k2 = PR.uniforms(seed, step, stream_id, i)
        for got, k in zip(out, (k1, k2)):
            assert 0 <= k < 2 ** 24 and got == k * 2.0 ** -24 and 0.0 <= got < 1.0      # k * 2^-24 is exact in fp32 and in a double
            assert got * 2.0 ** 24 == int(got * 2.0 ** 24)
    # the keying separates what it should: another seed, step, stream or element gives other words
    base = PR.words(seed, step, stream_id, 5)
    for other in (PR.words(seed + 1, step, stream_id, 5), PR.words(seed, step + 1, stream_id, 5), PR.words(seed, step, stream_id + 1, 5),
                  PR.words(seed, step, stream_id, 6)):
        assert other != base


def test_fill_gate_sets_every_field(built_lib):
    import torch
    from mga_yolo_amd import _binding, _lib
    p, out, msoft, gout, gp = (torch.zeros(2, 1, 3, 5) for _ in range(5))
    L = _lib.GateLevel()
    _binding.fill_gate(L, p, out, msoft, None, None, _lib.GATE_HARD_ST, 7, 0.3, 0.2, 0.6)
    got = {n: getattr(L, n) for n, _ in _lib.GateLevel._fields_}
    assert got == dict(p=p.data_ptr(), out=out.data_ptr(), msoft=msoft.data_ptr(), gout=None, gp=None, n=30, mode=2, stream_id=7,
                       tau=C.c_float(0.3).value, p_min=C.c_float(0.2).value, threshold=C.c_float(0.6).value)
    _binding.fill_gate(L, p, None, None, gout, gp, _lib.GATE_DETERMINISTIC, 0, 1.0, 0.0, 0.5)      # refilled for a backward: the forward's are cleared
    assert (L.out, L.msoft, L.gout, L.gp, L.mode, L.stream_id) == (None, None, gout.data_ptr(), gp.data_ptr(), 0, 0)


def _level(_lib, **over):
    L = _lib.GateLevel()
    for n in ("p", "out", "msoft", "gout", "gp"):
        setattr(L, n, P)
    L.n, L.mode, L.stream_id, L.tau, L.p_min, L.threshold = 64, _lib.GATE_GUMBEL, 0, 1.0, 0.0, 0.5
    for k, v in over.items():
        setattr(L, k, v)
    return L


STATE = 0x20000
CASES = [  # (what, overrides, expected code forward, expected code backward)  None = that direction does not look at it
    ("p NULL", dict(p=None), -1, -1), ("out NULL", dict(out=None), -1, None), ("msoft NULL in a soft mode", dict(msoft=None), -1, -1),
    ("gout NULL", dict(gout=None), None, -1), ("gp NULL", dict(gp=None), None, -1),
    ("n = 0", dict(n=0), -2, -2), ("tau = 0", dict(tau=0.0), -2, -2), ("tau < 0", dict(tau=-1.0), -2, -2), ("tau NaN", dict(tau=float("nan")), -2, -2),
    ("mode = 9", dict(mode=9), -2, -2), ("mode = -1", dict(mode=-1), -2, -2),
    ("p misaligned", dict(p=0x10002), -4, -4),
]


@pytest.mark.parametrize("what,over,fwd,bwd", CASES, ids=[c[0] for c in CASES])
def test_argument_errors_come_before_any_launch(built_lib, what, over, fwd, bwd):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for second in (False, True):                           # the bad level alone, and second of two: the first is not launched before it is found
        bad = _level(_lib, **over)
        arr = (_lib.GateLevel * 2)(_level(_lib), bad) if second else (_lib.GateLevel * 1)(bad)
        n = 2 if second else 1
        if fwd is not None:
            assert lib.mgagate_forward(arr, n, STATE, None) == fwd, what
            msg = lib.mgacbam_last_error().decode()
            assert msg.startswith("mgagate_forward") and f"level {n - 1}" in msg, msg
        if bwd is not None:
            assert lib.mgagate_backward(arr, n, None) == bwd, what
            msg = lib.mgacbam_last_error().decode()
            assert msg.startswith("mgagate_backward") and f"level {n - 1}" in msg, msg


def test_state_and_level_count_errors(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    arr = (_lib.GateLevel * 1)(_level(_lib))
    assert lib.mgagate_forward(arr, 1, STATE + 4, None) == _lib.E_ALIGN and b"8-byte" in lib.mgacbam_last_error()
    assert lib.mgagate_forward(arr, 1, None, None) == _lib.E_NULL and b"state" in lib.mgacbam_last_error()
    # a misaligned state is an error for a call of deterministic levels too
    det = (_lib.GateLevel * 1)(_level(_lib, mode=_lib.GATE_DETERMINISTIC, msoft=None))
    assert lib.mgagate_forward(det, 1, STATE + 4, None) == _lib.E_ALIGN
    for fn, extra in ((lib.mgagate_forward, (STATE,)), (lib.mgagate_backward, ())):
        assert fn(None, 1, *extra, None) == _lib.E_NULL
        assert fn(arr, 0, *extra, None) == _lib.E_LEVELS and fn(arr, _lib.MAX_LEVELS + 1, *extra, None) == _lib.E_LEVELS
        assert lib.mgacbam_last_error()


def test_gate_config():
    from mga_yolo_amd import GateConfig, _lib
    assert GateConfig().code() == _lib.GATE_GUMBEL and GateConfig("hard_st").code() == _lib.GATE_HARD_ST
    assert GateConfig("bernoulli_detach").code() == _lib.GATE_BERNOULLI_DETACH and GateConfig("deterministic").code() == _lib.GATE_DETERMINISTIC
    assert GateConfig("gumbel", training=False).code() == _lib.GATE_DETERMINISTIC          # an eval-mode gate returns the clamped input
    assert GateConfig().stream(2) == 2 and GateConfig(stream_id=5).stream(2) == 5
    with pytest.raises(ValueError):
        GateConfig("gumbell")
    with pytest.raises(ValueError):
        GateConfig(tau=0.0)


def test_plans_keep_their_argument_lists():
    """gate=None builds today's objects: the arguments every caller passes today are still there, in their order, and the two new ones are
    keywords at the end with defaults that switch the gate off."""
    from mga_yolo_amd.plan import PyramidPlan
    from mga_yolo_amd.slice import SlicePlan
    pp = list(inspect.signature(PyramidPlan.__init__).parameters.values())
    assert [p.name for p in pp] == ["self", "shapes", "params", "cfgs", "dtype", "device", "with_mask", "want_gmask", "use_proj", "fuse_forward",
                                    "grad_bucket", "gate", "seed"]
    sp = list(inspect.signature(SlicePlan.__init__).parameters.values())
    assert [p.name for p in sp] == ["self", "shapes", "hidden", "cbam_params", "cbam_cfgs", "head_states", "target_hw", "scale_weights", "bn_eps",
                                    "bn_momentum", "device", "training", "dtype", "gate", "seed"]
    for params in (pp, sp):
        assert params[-2].default is None and params[-1].default == 0
