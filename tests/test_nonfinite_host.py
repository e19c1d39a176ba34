"""CPU tests of what tests/test_gpu_nonfinite.py stands on (tests/nonfinite_cases.py):

  1. the autograd eager form of MaskSPADE (tests/spade_oracle.py: reference_form) equals the staged oracle on finite inputs;
  2. the eager forms of all four families reproduce the REFERENCE MODULES THEMSELVES on poisoned inputs: tests/golden/nonfinite_*.npz
     (oracle/gen_golden_nonfinite.py) hold, per poison, which elements of every output the reference left finite, and their values;
  3. every chosen row still has the launch form it was chosen for, and the restated channels-last rows are the tables' own;
  4. the rows' data: B >= 3, every element type on its rows, no MaskSPADE pre-activation on the ReLU edge, finite clean expectations, and
     the absorbed cases finite everywhere."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import nonfinite_cases as N
import spade_oracle as SO
from conftest import GOLDEN, rel_err

NAMES = {"cbam": {"cam_mlp.0.weight": "w1", "cam_mlp.0.bias": "b1", "cam_mlp.2.weight": "w2", "cam_mlp.2.bias": "b2", "sam_conv.weight": "wsa",
                  "beta": "beta"},
         "eca": {"conv1d.weight": "w", "beta": "beta"},
         "head": {"proj.0.weight": "w1", "proj.1.weight": "gamma", "proj.1.bias": "beta", "head.weight": "wh", "head.bias": "bh"},
         "spade": {k: k for k in SO.PARAM_KEYS}}


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the MaskSPADE eager form against the staged oracle, finite inputs
# ---------------------------------------------------------------------------------------------------------------------------
SPADE_ROWS = [r for r in N.ROWS if r.family == "spade"]


@pytest.mark.parametrize("r", SPADE_ROWS, ids=[N.row_id(r) for r in SPADE_ROWS])
def test_spade_eager_form_equals_the_staged_oracle(r):
    """Both in fp64 on the same inputs: they differ by the order of fp64 sums only, 1e-9 of each tensor's scale (the margin the CBAM and ECA
    rows give their two oracles, cbam_nchw_rows.row_case).  Batch norm: the updated running statistics too."""
    c = N.case(r, "f32")
    inp = c.inp
    run = inp.get("running")
    y, ctx = SO.forward(inp["x"], inp["mask"], inp["params"], c.cfg["norm_type"], True, c.use_sig, c.cfg["eps"], run, c.cfg["momentum"])
    g = SO.backward(inp["gy"], ctx)
    assert SO.min_abs_pre(ctx) >= 1e-5
    want = N.expected(c)
    assert rel_err(want["y"], y) < 1e-9
    for k in ("gx", "gmask"):
        assert rel_err(want[k], g[k]) < 1e-9, k
    for k in SO.PARAM_KEYS:
        assert want["g." + k].shape == g[k].shape and rel_err(want["g." + k], g[k]) < 1e-9, k
    if run is not None:
        for k, w in zip(("running_mean", "running_var"), ctx["new_running"]):
            assert rel_err(want[k], w) < 1e-9, k
        assert torch.equal(inp["running"][0], torch.zeros_like(run[0])), "the case's running statistics were written to"


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the eager forms against the reference modules' own record
# ---------------------------------------------------------------------------------------------------------------------------
def _load(family):
    z = np.load(os.path.join(GOLDEN, f"nonfinite_{family}.npz"), allow_pickle=False)
    return z, json.loads(bytes(z["meta"]).decode())


def _golden_cases():
    out = []
    for family in N.FAMILIES:
        _, meta = _load(family)
        out += [(family, name, p["id"]) for name, m in meta.items() for p in m["poisons"]]
    return out


def _golden_inputs(family, z, meta, name, poison):
    """-> (a case as nonfinite_cases.eager_step takes it, its inputs with the poison in place)"""
    m = meta[name]
    state = {k[len(name) + len(".param."):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{name}.param.")}
    params = {short: state[ref].clone() for ref, short in NAMES[family].items()}
    cfg = dict(m["cfg"])
    if family == "head":
        params["w1"] = params["w1"].reshape(params["w1"].shape[:2])
        cfg["training"] = m["training"]
    inp = dict(x=torch.from_numpy(z[f"{name}.x"]).clone(), gy=torch.from_numpy(z[f"{name}.gy"]).clone(),
               mask=torch.from_numpy(z[f"{name}.mask"]).clone() if m["has_mask"] else None, params=params)
    run = [k for k in state if k.endswith("running_mean")]
    if run and (family == "head" or cfg.get("norm_type") == "bn"):
        inp["running"] = (state[run[0]].clone(), state[run[0].replace("running_mean", "running_var")].clone())
    if poison["target"] in ("x", "mask", "gy"):
        inp[poison["target"]][tuple(poison["index"])] = float(poison["value"])
    elif poison["target"] is not None:
        t = params[NAMES[family][poison["target"]]]
        t[tuple(poison["index"][:t.dim()])] = float(poison["value"])
    return SimpleNamespace(family=family, cfg=cfg), inp


@pytest.mark.parametrize("family,name,pid", _golden_cases(), ids=["-".join(c) for c in _golden_cases()])
def test_eager_forms_reproduce_the_reference_modules_under_poison(family, name, pid):
    """The eager form runs in fp32, as the reference did: the same ATen operators on the same values, so the finite-masks are the
    reference's exactly, and the finite values differ by the order of fp32 sums at most -- 1e-5 of the scale of each tensor's finite part
    (a hundred roundings of 2^-24; the goldens' sums run over 30 to 720 terms)."""
    z, meta = _load(family)
    (poison,) = [p for p in meta[name]["poisons"] if p["id"] == pid]
    c, inp = _golden_inputs(family, z, meta, name, poison)
    got = N.eager_step(c, inp, torch.float32)
    want = {}
    for k in z.files:
        if k.startswith(f"{name}.{pid}.finite."):
            key = k[len(f"{name}.{pid}.finite."):]
            short = ("g." + NAMES[family][key[2:]]) if key.startswith("g.") else (key[key.index("running_"):] if key.startswith("after.") else key)
            want[short] = (torch.from_numpy(z[k]), torch.from_numpy(z[f"{name}.{pid}.value.{key}"]))
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    report = []
    for k, (fin, val) in want.items():
        g = got[k].reshape(fin.shape)
        if not torch.equal(torch.isfinite(g), fin):
            report.append(f"{k}: finite where the reference is not, or the reverse, at {int((torch.isfinite(g) != fin).sum())} of {fin.numel()} elements")
        elif bool(fin.any()):
            e = float((g - val).abs()[fin].max() / val.abs()[fin].max().clamp_min(1e-30))
            if not e < 1e-5:
                report.append(f"{k}: {e:.3e}")
    assert not report, report


def test_goldens_are_no_larger_than_the_largest_committed_one():
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)}
    largest_other = max(v for f, v in sizes.items() if not f.startswith("nonfinite_"))
    assert all(v <= largest_other for f, v in sizes.items() if f.startswith("nonfinite_")), sizes


# ---------------------------------------------------------------------------------------------------------------------------
# 3. launch forms
# ---------------------------------------------------------------------------------------------------------------------------
FORM_CASES = [(r, dt) for r in N.ROWS for dt in r.dtypes]


@pytest.mark.parametrize("r,dt", FORM_CASES, ids=[f"{N.row_id(r)}-{dt}" for r, dt in FORM_CASES])
def test_row_has_the_launch_form_it_was_chosen_for(r, dt):
    g, want = N.row_geometry(r, dt), N.form_of(r, dt)
    assert {k: g[k] for k in want} == want, r.what


def test_the_forms_the_issue_names_are_all_there():
    """MaskCBAM: fused gate launch and the three-launch fallback, pool_forms_ca and the staged / split MLP, merged and unmerged backward,
    projection planes narrow, wide and off; MaskECA: the role-workgroup backward with every tap role; MaskSPADE: every hidden width and
    a channel tail; the head: fp32 and half MFMA forms; every family in both layouts, fp32 and fp16 everywhere, bf16 once per family."""
    geo = {(N.row_id(r), dt): N.row_geometry(r, dt) for r, dt in FORM_CASES}
    cb = [g for (rid, dt), g in geo.items() if rid.startswith("cbam-nchw")]
    for key, values in dict(gate=(True, False), pool_ca=(True, False), stream=(True, False), split_mlp=(True, False), merge=(True, False),
                            fold=(True, False), make_proj=(0, 1, 2)).items():
        assert {g[key] for g in cb} >= set(values), key
    assert any(r.family == "eca" and N.case(r, "f32").cfg["k"] == 15 for r in N.ROWS)
    sp = [N.spade_case(r) for r in N.ROWS if r.family == "spade"]
    assert {c.hidden for c in sp} == {16, 32, 48, 64} and any(c.C % 32 == 16 for c in sp) and {c.norm for c in sp} == {"in", "bn"}
    hd = {(dt, geo[(N.row_id(r), dt)]["fw_w"]) for r in N.ROWS if r.family == "head" and r.layout == "nchw" for dt in r.dtypes}
    assert {("f32", "guard"), ("f16", "guard"), ("f16", "gather")} <= hd         # fp32 MFMAs, half MFMAs, fp32 MFMAs on half features
    for family in N.FAMILIES:
        rows = [r for r in N.ROWS if r.family == family]
        assert {lay for r in rows for lay in N.layouts(r)} == {"nchw", "nhwc"}, family
        assert all({"f32"} <= set(r.dtypes) or {"f16"} <= set(r.dtypes) for r in rows) and any("bf16" in r.dtypes for r in rows), family
        assert all(r.B >= 3 for r in rows), family


def test_restated_channels_last_rows_are_the_tables_own():
    from test_gpu_channels_last_edges import EDGE_ROWS
    from test_gpu_eca_channels_last import ECA_EDGE_ROWS
    for mine, table in ((N.CBAM_NHWC, EDGE_ROWS), (N.ECA_NHWC, ECA_EDGE_ROWS)):
        rows = {t[0]: t for t in table}
        for name, (B, C, H, W, k, kind, mask3d) in mine.items():
            assert rows[name][2:9] == (B, C, H, W, k, kind, mask3d), name


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the rows' data
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", N.ROWS, ids=[N.row_id(r) for r in N.ROWS])
def test_row_data(r):
    """The clean expectation is finite; every poison makes something non-finite unless it is an absorbed case, which leaves everything
    finite; the poisoned sample is the middle one and B >= 3 leaves a clean sample on either side."""
    dt = r.dtypes[-1]
    for training in ((True, False) if r.family == "head" else (True,)):
        c = N.case(r, dt, training)
        assert c.B == r.B >= 3 and c.inp["x"].shape[0] == c.B and 0 < c.B // 2 < c.B - 1
        assert torch.equal(c.inp["x"], c.inp["x"].to(c.dtype).float()) and torch.equal(c.inp["gy"], c.inp["gy"].to(c.dtype).float())
        assert all(bool(torch.isfinite(v).all()) for v in N.expected(c).values())
        for p in N.poisons_of(c):
            nonfinite = sum(int((~torch.isfinite(v)).sum()) for v in N.expected(c, p).values())
            assert (nonfinite == 0) == N.absorbed(c, p), (p.id, nonfinite)
        if r.family == "spade":                                        # no ReLU branch can differ on the device, clean or absorbed
            for p in [None] + [q for q in N.poisons_of(c) if N.absorbed(c, q)]:
                inp = c.inp if p is None else N.poisoned(c, p)
                _, ctx = SO.forward(inp["x"], inp["mask"], inp["params"], c.cfg["norm_type"], True, c.use_sig, c.cfg["eps"], inp.get("running"),
                                    c.cfg["momentum"])
                assert SO.min_abs_pre(ctx) >= 1e-5, (N.row_id(r), None if p is None else p.id, SO.min_abs_pre(ctx))
