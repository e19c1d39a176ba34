"""CPU-side checks of the fused optimizer's entry points (include/mgaopt.h) on the built library: every argument error -- each returned
before anything is launched (there is no GPU here) -- and the chunk table mgaopt_ws_init builds.  The header against the binding is
tests/test_abi_headers.py's."""
import ctypes as C
import inspect

import pytest

from abi_header import FAKE as P


def test_fill_opt_segment_sets_every_field(built_lib):
    import torch
    from mga_yolo_amd import _binding, _lib
    p, g, s0, s1, e = (torch.zeros(3, 5) for _ in range(5))
    S = _lib.OptSegment()
    S.reserved = 9
    _binding.fill_opt_segment(S, p, g, s0, s1, e, 2)
    assert {n: getattr(S, n) for n, _ in _lib.OptSegment._fields_} == dict(param=p.data_ptr(), grad=g.data_ptr(), state0=s0.data_ptr(),
                                                                          state1=s1.data_ptr(), ema=e.data_ptr(), n=15, group=2, reserved=0)
    _binding.fill_opt_segment(S, p, None, None, None, e, 1)                       # refilled as an EMA-only segment: the others are cleared
    assert (S.grad, S.state0, S.state1, S.ema, S.group) == (None, None, None, e.data_ptr(), 1)


HYPER, WS = 0x20000, 0x30000


def _seg(_lib, **over):
    S = _lib.OptSegment()
    for n in ("param", "grad", "state0", "state1", "ema"):
        setattr(S, n, P)
    S.n, S.group = 1500, 1
    for k, v in over.items():
        setattr(S, k, v)
    return S


def _cfg(_lib, **over):
    K = _lib.OptCfg(_lib.OPT_ADAMW, 1, 0, 0, 0.999, 1e-8, 10.0, 0.9999, 2000.0)
    for k, v in over.items():
        setattr(K, k, v)
    return K


SEG_CASES = [  # (what, overrides, code from mgaopt_step with AdamW, is it refused by the size query as well)
    ("param NULL", dict(param=None), -1, True), ("state0 NULL", dict(state0=None), -1, True),
    ("state1 NULL for AdamW", dict(state1=None), -1, False),
    ("neither grad nor ema", dict(grad=None, ema=None), -1, True),
    ("n = 0", dict(n=0), -2, True), ("n < 0", dict(n=-5), -2, True), ("n = 2^31", dict(n=2 ** 31), -2, True),
    ("group = 3", dict(group=3), -2, True), ("group = -1", dict(group=-1), -2, True),
    ("param misaligned", dict(param=P + 2), -4, True), ("grad misaligned", dict(grad=P + 1), -4, True),
    ("state0 misaligned", dict(state0=P + 2), -4, True), ("state1 misaligned", dict(state1=P + 3), -4, True), ("ema misaligned", dict(ema=P + 2), -4, True),
]


@pytest.mark.parametrize("what,over,code,sized", SEG_CASES, ids=[c[0] for c in SEG_CASES])
def test_segment_errors_come_before_any_launch(built_lib, what, over, code, sized):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    for second in (False, True):                           # the bad segment alone, and second of two
        bad = _seg(_lib, **over)
        arr = (_lib.OptSegment * 2)(_seg(_lib), bad) if second else (_lib.OptSegment * 1)(bad)
        n = 2 if second else 1
        assert lib.mgaopt_step(arr, n, C.byref(_cfg(_lib)), HYPER, WS, 1 << 20, None) == code, what
        msg = lib.mgacbam_last_error().decode()
        assert msg.startswith("mgaopt_step") and f"segment {n - 1}" in msg, msg
        assert (lib.mgaopt_ws_bytes(arr, n) == 0) == sized, what
    # a segment SGD accepts without state1, and an EMA-only one without grad and state
    ok = (_lib.OptSegment * 2)(_seg(_lib, state1=None), _seg(_lib, grad=None, state0=None, state1=None))
    assert lib.mgaopt_ws_bytes(ok, 2) > 0


def test_call_errors_come_before_any_launch(built_lib):
    from mga_yolo_amd import _lib
    lib = _lib.load()
    arr = (_lib.OptSegment * 1)(_seg(_lib))
    need = lib.mgaopt_ws_bytes(arr, 1)
    # [segments 56 -> 64][2 chunks x 16][2 partials -> 16][2 flags -> 16]
    assert need == 64 + 32 + 16 + 16
    step = lambda segs=arr, n=1, cfg=None, hyper=HYPER, ws=WS, nbytes=need: lib.mgaopt_step(segs, n, C.byref(cfg or _cfg(_lib)), hyper, ws, nbytes, None)
    err = lambda: lib.mgacbam_last_error().decode()
    assert step(segs=None) == _lib.E_NULL and "segs" in err()
    assert step(n=0) == _lib.E_LEVELS and step(n=_lib.OPT_MAX_SEGMENTS + 1) == _lib.E_LEVELS and "n_segs" in err()
    assert lib.mgaopt_step(arr, 1, None, HYPER, WS, need, None) == _lib.E_NULL and "cfg" in err()
    assert step(hyper=None) == _lib.E_NULL and "hyper" in err()
    assert step(hyper=HYPER + 4) == _lib.E_ALIGN and "8-byte" in err()
    assert step(ws=None) == _lib.E_NULL and "ws" in err()
    assert step(ws=WS + 8) == _lib.E_ALIGN and "16-byte" in err()
    assert step(nbytes=need - 1) == _lib.E_SIZE and "ws holds" in err()
    for over in (dict(kind=2), dict(kind=-1), dict(max_norm=0.0), dict(max_norm=float("nan")), dict(beta2=1.0), dict(beta2=0.0), dict(eps=-1.0),
                 dict(ema_tau=0.0), dict(ema_decay=1.5)):
        assert step(cfg=_cfg(_lib, **over)) == _lib.E_SHAPE, over
        assert err().startswith("mgaopt_step")
    assert lib.mgaopt_ws_bytes(None, 1) == 0 and lib.mgaopt_ws_bytes(arr, 0) == 0
    # the accumulate launch
    assert lib.mgaopt_accumulate(None, P, 8, None) == _lib.E_NULL and lib.mgaopt_accumulate(P, None, 8, None) == _lib.E_NULL
    assert lib.mgaopt_accumulate(P, P, 0, None) == _lib.E_SHAPE
    assert lib.mgaopt_accumulate(P + 2, P, 8, None) == _lib.E_ALIGN and lib.mgaopt_accumulate(P, P + 1, 8, None) == _lib.E_ALIGN
    assert err().startswith("mgaopt_accumulate")
    # the table image
    buf = (C.c_uint8 * need)()
    assert lib.mgaopt_ws_init(arr, 1, None, need) == _lib.E_NULL
    assert lib.mgaopt_ws_init(arr, 1, buf, need - 1) == _lib.E_SIZE
    assert lib.mgaopt_ws_init((_lib.OptSegment * 1)(_seg(_lib, n=0)), 1, buf, need) == _lib.E_SHAPE


def test_chunk_table(built_lib):
    """One (segment, offset, length <= 1024) entry per workgroup, in the order of the segments; the segment list itself in front."""
    import numpy as np
    from mga_yolo_amd import _lib
    lib = _lib.load()
    lengths = [1, 2, 147, 1023, 1024, 1025, 4099, 65]
    arr = (_lib.OptSegment * len(lengths))(*[_seg(_lib, n=n, group=i % 3, param=P + 4 * i) for i, n in enumerate(lengths)])
    need = lib.mgaopt_ws_bytes(arr, len(lengths))
    chunks = sum((n + 1023) // 1024 for n in lengths)
    assert chunks == 13
    pad16 = lambda b: (b + 15) // 16 * 16
    assert need == pad16(56 * len(lengths)) + 16 * chunks + 2 * pad16(4 * chunks)
    buf = (C.c_uint8 * need)()
    assert lib.mgaopt_ws_init(arr, len(lengths), buf, need) == 0
    raw = bytes(buf)
    assert raw[:56 * len(lengths)] == bytes(arr)
    tab = np.frombuffer(raw, dtype=np.int32, count=4 * chunks, offset=pad16(56 * len(lengths))).reshape(chunks, 4)
    want = [(s, off, min(1024, n - off), 0) for s, n in enumerate(lengths) for off in range(0, n, 1024)]
    assert [tuple(r) for r in tab.tolist()] == want
    assert all(0 < ln <= 1024 and off + ln <= lengths[s] for s, off, ln, _ in want)          # no chunk reaches past its segment


def test_public_names_and_unchanged_plan_arguments():
    import mga_yolo_amd as M
    from mga_yolo_amd.optim import BucketOptimizer
    for name in ("OptConfig", "BucketOptimizer"):
        assert name in M.__all__ and hasattr(M, name)
    assert [p for p in inspect.signature(BucketOptimizer.for_plan).parameters] == ["plan", "cfg", "ema", "accumulate"]
    assert [p for p in inspect.signature(BucketOptimizer.__init__).parameters][:4] == ["self", "segments", "cfg", "device"]
    assert list(inspect.signature(M.SlicePlan.create).parameters) == ["shapes", "hidden", "block_params", "block_cfgs", "head_states", "block",
                                                                      "channels_last", "target_resize", "block_running", "kw"]
