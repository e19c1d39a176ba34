"""The C ABI, header by header: every record of mga_yolo_amd._lib.HEADERS against the file under include/ it describes (read by
tests/abi_header.py), against the built library, against the C compiler, and against the literals of PINNED below.  The record and the
header are two statements of one ABI and are compared in full; PINNED is the third, written by hand, so that a header and its mirror
changed together still fail here.  No kernel is launched.  What a family's own test file keeps is its behaviour: size arithmetic, refusals
and their messages, the fill functions."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import pytest

import abi_header as A
from conftest import ROOT
from mga_yolo_amd import _lib

NAMES = tuple(_lib.HEADERS)
MAIN_HEADER_SHA256 = "3ccfaba7fad40504a8863d384a7e48c82381155d39af6e43f3382dccbc9c7715"       # include/mgacbam.h at ABI 15


def _tail(names, offsets):
    return dict(zip(names.split(), offsets))


# By hand (LP64).  symbols: the header's functions, sorted.  constants: every named integer.  layouts: tag -> (sizeof, {field: offset})
# of the struct's LAST fields, in order -- all of them where every field is listed.
PINNED = {
    "mgacbam.h": dict(
        symbols=["mgacbam_abi_version", "mgacbam_backward", "mgacbam_backward_stages", "mgacbam_build_info", "mgacbam_bwd_scratch_bytes",
                 "mgacbam_bwd_scratch_bytes_flags", "mgacbam_ctx_bytes", "mgacbam_ctx_layout", "mgacbam_eca_backward", "mgacbam_eca_ctx_bytes",
                 "mgacbam_eca_ctx_bytes_flags", "mgacbam_eca_forward", "mgacbam_eca_scratch_bytes", "mgacbam_eca_scratch_bytes_flags",
                 "mgacbam_forward", "mgacbam_forward_stages", "mgacbam_fwd_ws_bytes", "mgacbam_last_error", "mgacbam_reload_env",
                 "mgacbam_resize_nearest", "mgahead_backward", "mgahead_bwd_scratch_bytes", "mgahead_bwd_scratch_bytes_flags", "mgahead_ctx_bytes",
                 "mgahead_ctx_bytes_flags", "mgahead_forward", "mgakendall_backward", "mgakendall_forward", "mgapmg_backward", "mgapmg_forward",
                 "mgaseg_backward", "mgaseg_forward", "mgaseg_kendall_backward", "mgaseg_kendall_forward", "mgaseg_ws_bytes"],
        constants=dict(MGACBAM_ABI_VERSION=15, MGACBAM_MAX_LEVELS=8, MGACBAM_F32=0, MGACBAM_F16=1, MGACBAM_BF16=2, MGACBAM_PROJ_MAX_HIDDEN=4,
                       MGACBAM_FWD_SAVE_PROJ=1, MGACBAM_BWD_HAVE_PROJ=1, MGACBAM_LAYOUT_NHWC=2,
                       MGACBAM_E_NULL=-1, MGACBAM_E_SHAPE=-2, MGACBAM_E_DTYPE=-3, MGACBAM_E_ALIGN=-4, MGACBAM_E_LEVELS=-5, MGACBAM_E_SIZE=-6,
                       MGACBAM_FWD_POOL=1, MGACBAM_FWD_CHAN=2, MGACBAM_FWD_APPLY=4, MGACBAM_FWD_ALL=7, MGACBAM_FWD_FUSE=8,
                       MGACBAM_BWD_REDUCE1=1, MGACBAM_BWD_CONVT=2, MGACBAM_BWD_REDUCE2=4, MGACBAM_BWD_WSA=8, MGACBAM_BWD_PARAMGRAD=16,
                       MGACBAM_BWD_APPLY=32, MGACBAM_BWD_FUSE=64, MGACBAM_BWD_PARAMS=31, MGACBAM_BWD_INPUTS=32, MGACBAM_BWD_ALL=127,
                       MGACBAM_BWD_FOLD=128, MGASEG_MAX_LEVELS=4, MGASEG_NEAREST=0, MGASEG_BILINEAR=1,
                       MGAHEAD_BWD_ACCUM_GX=1, MGAHEAD_LOGITS_F32=2, MGAHEAD_LAYOUT_NHWC=4),
        layouts=dict(
            # the workspace travels last; the 8 pointers / sizes and the 72-byte params in front, then six int32
            mgacbam_fwd_level=(152, _tail("flags ws ws_bytes", (132, 136, 144))),
            # flags is the last field, dtype before it: it took the 4 bytes of tail padding, so the sizes are those from before it existed
            mgacbam_eca_fwd_level=(96, _tail("dtype flags", (88, 92))),
            mgacbam_eca_bwd_level=(144, _tail("dtype flags", (136, 140))))),
    "mgaspade.h": dict(
        symbols=["mgaspade_backward", "mgaspade_ctx_bytes", "mgaspade_forward", "mgaspade_scratch_bytes"],
        constants=dict(MGASPADE_NORM_IN=0, MGASPADE_NORM_BN=1, MGASPADE_LAYOUT_NHWC=2),
        # 25 eight-byte members (21 pointers, ctx, ctx_bytes, scratch, scratch_bytes), then 13 four-byte ones, padded to 8
        layouts=dict(mgaspade_level=(256, _tail(
            "x mask y gy gx gmask w0 b0 wg bg wb bb running_mean running_var num_batches_tracked gw0 gb0 gwg gbg gwb gbb ctx ctx_bytes scratch "
            "scratch_bytes B C H W hidden dtype norm_type training use_sigmoid_mask save_gamma eps momentum flags",
            [8 * i for i in range(25)] + [200 + 4 * i for i in range(13)])))),
    "mgaresample.h": dict(
        symbols=["mgaspade_resample_backward", "mgaspade_resample_forward"],
        constants={},
        # two pointers, five four-byte members, padded to 8
        layouts=dict(mgaspade_resample_level=(40, _tail("src dst B in_h in_w out_h out_w", (0, 8, 16, 20, 24, 28, 32))))),
    "mgagate.h": dict(
        symbols=["mgagate_backward", "mgagate_forward", "mgagate_philox4x32", "mgagate_uniforms"],
        constants=dict(MGAGATE_DETERMINISTIC=0, MGAGATE_GUMBEL=1, MGAGATE_HARD_ST=2, MGAGATE_BERNOULLI_DETACH=3),
        # five pointers, then six four-byte members
        layouts=dict(mgagate_level=(64, _tail("p out msoft gout gp n mode stream_id tau p_min threshold", (0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60))))),
    "mgaopt.h": dict(
        symbols=["mgaopt_accumulate", "mgaopt_step", "mgaopt_ws_bytes", "mgaopt_ws_init"],
        constants=dict(MGAOPT_SGD=0, MGAOPT_ADAMW=1, MGAOPT_GROUPS=3, MGAOPT_MAX_SEGMENTS=4096, MGAOPT_CHUNK=1024),
        layouts=dict(
            mgaopt_segment=(56, _tail("param grad state0 state1 ema n group reserved", (0, 8, 16, 24, 32, 40, 48, 52))),
            mgaopt_cfg=(56, _tail("kind check_finite zero_grad reserved beta2 eps max_norm ema_decay ema_tau", (0, 4, 8, 12, 16, 24, 32, 40, 48))),
            mgaopt_hyper=(128, _tail("lr momentum one_minus_momentum ln_momentum weight_decay inv_scale ext_sumsq ext_found_inf updates t grad_norm "
                                     "clip_coef found_inf reserved", [4 * w for w in (0, 3, 6, 9, 12, 15, 16, 17, 18, 19, 21, 22, 23, 24)])))),
    "mgatargets.h": dict(
        symbols=["mgatgt_forward", "mgatgt_scratch_bytes"],
        constants=dict(MGACBAM_E_ARG=-7, MGATGT_AVGPOOL=0, MGATGT_MAXPOOL=1, MGATGT_SRC_U8=0, MGATGT_SRC_F32=1, MGATGT_CLOSE3=1, MGATGT_MAX_LEVELS=4),
        # src, dst[4] -- five pointers; stride[4] and eight more int32; scratch, scratch_bytes
        layouts=dict(mgatgt_desc=(104, dict(src=0, dst=8, stride=40, n_levels=56, B=60, H=64, W=68, src_dtype=72, method=76, flags=80, reserved=84,
                                            scratch=88, scratch_bytes=96)))),
    "mgadet.h": dict(
        symbols=["mgadet_backward", "mgadet_forward", "mgadet_ws_bytes"],
        constants=dict(MGADET_MAX_LEVELS=4, MGADET_MAX_TOPK=16, MGADET_MAX_GT=256),
        # 2 x 4 pointers; 3 x 4 int32; 8 int32; 3 floats + 1 int32; 10 pointers; ws, ws_bytes
        layouts=dict(mgadet_desc=(256, dict(feats=0, g_feats=32, H=64, W=80, stride=96, n_levels=112, B=116, nc=120, reg_max=124, dtype=128, topk=132,
                                            n_cap=136, m_cap=140, gains=144, reserved=156, batch_idx=160, cls=168, bboxes=176, n=184, assign_gt=192,
                                            assign_score=200, out=208, items=216, status=224, upstream=232, ws=240, ws_bytes=248)))),
    "mganms.h": dict(
        symbols=["mganms_run", "mganms_ws_bytes"],
        constants=dict(MGANMS_MAX_LEVELS=4, MGANMS_MULTI_LABEL=1, MGANMS_AGNOSTIC=2),
        # 4 + 1 pointers; 3 x 4 int32; 8 int32; 2 floats; 2 int32; 4 pointers; ws, ws_bytes
        layouts=dict(mganms_desc=(184, dict(feats=0, pred=32, H=40, W=56, stride=72, n_levels=88, A=92, B=96, nc=100, dtype=104, max_det=108,
                                            max_nms=112, flags=116, conf_thres=120, iou_thres=124, cand_cap=128, reserved=132, dets=136, count=144,
                                            keep=152, status=160, ws=168, ws_bytes=176)))),
}


def test_the_table_covers_every_header_under_include():
    assert sorted(NAMES) == A.headers() == sorted(PINNED)


@pytest.mark.parametrize("name", NAMES)
def test_symbols_declared_bound_and_exported(built_lib, name):
    declared, bound = sorted(A.read(name).functions), sorted(_lib.HEADERS[name].symbols)
    assert declared == bound, f"{name}: declared but not bound {sorted(set(declared) - set(bound))}, bound but not declared {sorted(set(bound) - set(declared))}"
    assert bound == PINNED[name]["symbols"], f"{name}: symbols differ from the pinned list: {sorted(set(bound) ^ set(PINNED[name]['symbols']))}"
    raw = C.CDLL(built_lib)
    for fn in declared:
        assert hasattr(raw, fn), f"{name}: {fn} is declared but the library does not export it"
    others = {fn for other, rec in _lib.HEADERS.items() if other != name for fn in rec.symbols}
    assert not set(bound) & others, f"{name}: {sorted(set(bound) & others)} bound by another record as well"


@pytest.mark.parametrize("name", NAMES)
def test_constants_equal_the_header_s(name):
    declared, mirrored, pinned = A.read(name).constants, _lib.HEADERS[name].constants, PINNED[name]["constants"]
    assert sorted(declared) == sorted(mirrored) == sorted(pinned), \
        f"{name}: constants without a mirror {sorted(set(declared) - set(mirrored))}, mirrors without a constant {sorted(set(mirrored) - set(declared))}, " \
        f"pinned otherwise {sorted(set(pinned) ^ set(declared))}"
    for k, v in declared.items():
        assert mirrored[k] == v, f"{name}: {k} is {v} in the header, {mirrored[k]} in _lib"
        assert pinned[k] == v, f"{name}: {k} is {v} in the header, pinned as {pinned[k]}"


@pytest.mark.parametrize("name", NAMES)
def test_struct_mirrors_equal_the_header_s(name):
    """Tags, field names and order, every field's C type, every offset and sizeof: mirror == the header's own types laid out by ctypes ==
    (where there is a C compiler) what a program that includes every header prints.  Names alone do not see a wrong width or a missed
    padding; offsets alone do not see an int32 mirrored as a float."""
    parsed, mirrors = A.read(name).structs, _lib.HEADERS[name].structs
    assert sorted(parsed) == sorted(mirrors), f"{name}: structs without a mirror {sorted(set(parsed) - set(mirrors))}, mirrors without a struct {sorted(set(mirrors) - set(parsed))}"
    compiled = A.compiler_layout(NAMES)
    for tag, fields in parsed.items():
        M, H = mirrors[tag], A.ctypes_from_header(tag)
        declared, mirrored = [f for _, f, _ in fields], [f[0] for f in M._fields_]
        differ = [f"field {i} is {h} in the header, {m} in the mirror" for i, (h, m) in enumerate(zip(declared, mirrored)) if h != m]
        assert declared == mirrored, f"{name}: {tag}: {differ[0] if differ else f'{len(declared)} fields in the header, {len(mirrored)} in the mirror'}"
        for (field, tm), (_, th) in zip(M._fields_, H._fields_):
            assert A.same_ctype(tm, th), f"{name}: {tag}.{field} is {th.__name__} in the header, {tm.__name__} in the mirror"
        (size, offsets), (hsize, hoffsets) = A.layout(M), A.layout(H)
        for field in offsets:
            assert offsets[field] == hoffsets[field], f"{name}: {tag}.{field} at {offsets[field]} in the mirror, {hoffsets[field]} by the header's types"
        assert size == hsize, f"{name}: sizeof({tag}_t) is {hsize} by the header's types, {size} in the mirror"
        assert bytes(M()) == bytes(size), f"{name}: {tag}: a fresh mirror is not zero-filled"          # flags == 0: the behaviour before a flag existed
        if compiled is not None:
            csize, coffsets = compiled[tag]
            for field in offsets:
                assert offsets[field] == coffsets[field], f"{name}: {tag}.{field} at {offsets[field]} in the mirror, {coffsets[field]} by the compiler"
            assert size == csize, f"{name}: sizeof({tag}_t) is {csize} by the compiler, {size} in the mirror"


@pytest.mark.parametrize("name", NAMES)
def test_struct_mirrors_keep_the_pinned_layout(name):
    mirrors = _lib.HEADERS[name].structs
    assert set(PINNED[name]["layouts"]) <= set(mirrors), name
    for tag, (size, tail) in PINNED[name]["layouts"].items():
        got_size, offsets = A.layout(mirrors[tag])
        assert list(offsets)[-len(tail):] == list(tail), f"{name}: {tag}: the last fields are {list(offsets)[-len(tail):]}, pinned as {list(tail)}"
        for field, off in tail.items():
            assert offsets[field] == off, f"{name}: {tag}.{field} at {offsets[field]}, pinned at {off}"
        assert got_size == size, f"{name}: sizeof({tag}_t) is {got_size}, pinned as {size}"
    if name == "mgatargets.h":
        assert (_lib.TargetsDesc.dst.size, _lib.TargetsDesc.stride.size) == (32, 16)


def test_abi_version_and_build_info(built_lib):
    lib = _lib.load()
    assert A.read("mgacbam.h").constants["MGACBAM_ABI_VERSION"] == _lib.ABI_VERSION == lib.mgacbam_abi_version() == 15
    assert b"gfx950" in lib.mgacbam_build_info()


def test_name_maps():
    """The dicts callers index by a module's own option names"""
    assert _lib.GATE_MODES == dict(deterministic=0, gumbel=1, hard_st=2, bernoulli_detach=3)
    assert _lib.OPT_KINDS == dict(sgd=0, adamw=1) and _lib.TGT_METHODS == dict(avgpool=0, maxpool=1)
    assert _lib.FWD_STAGES == dict(pool=1, chan=2, apply=4) and _lib.BWD_STAGES == dict(reduce1=1, convT=2, reduce2=4, wsa=8, params=16, apply=32)


def test_main_header_is_byte_identical():
    """include/mgacbam.h hashes to what it did before the first header beside it existed, and (where the checkout has its history) to the
    committed one."""
    path = os.path.join(ROOT, "include", "mgacbam.h")
    have = hashlib.sha256(open(path, "rb").read()).hexdigest()
    assert have == MAIN_HEADER_SHA256
    git = shutil.which("git")
    if git and os.path.exists(os.path.join(ROOT, ".git")):
        r = subprocess.run([git, "-C", ROOT, "show", "HEAD:include/mgacbam.h"], capture_output=True)
        if r.returncode == 0:                                  # (a checkout git refuses to read, e.g. another user's, leaves the pinned hash)
            assert hashlib.sha256(r.stdout).hexdigest() == have


def test_the_later_headers_are_additive():
    """Each family after MaskECA came as a header of its own: the main header names none of them, and what they share they include."""
    main = A.read("mgacbam.h")
    raw = open(os.path.join(ROOT, "include", "mgacbam.h")).read()
    for word in ("mgaspade_level", "mgatgt", "MGACBAM_E_ARG", "mgadet", "mganms"):
        assert word not in main.text, word
    for word in ("mgagate", "mgaopt"):
        assert word not in raw, word                           # not even in a comment
    assert main.includes == ()
    assert "mgaresample.h" in A.read("mgaspade.h").includes    # one include serves MaskSPADE's callers
    for name in ("mgadet.h", "mganms.h"):                      # MGACBAM_E_ARG is reused through the include, not redefined
        assert "mgatargets.h" in A.read(name).includes and "MGACBAM_E_ARG" not in A.read(name).constants and "MGACBAM_E_ARG =" not in A.read(name).text
    codes = [v for k, v in {**main.constants, **A.read("mgatargets.h").constants}.items() if k.startswith("MGACBAM_E_")]
    assert sorted(codes) == [-7, -6, -5, -4, -3, -2, -1]
