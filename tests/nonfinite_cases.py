"""What tests/test_nonfinite_host.py and tests/test_gpu_nonfinite.py share.  Not a test.

The rule under test ("Non-finite values"): a NaN or an infinity that enters a block -- in the feature map, a mask logit, the
upstream gradient or a parameter -- comes out non-finite wherever the reference's torch operators would carry it, and nowhere else.

  1. ROWS: per family and layout the smallest row of each launch form of the family's own row table, with B >= 3 (widened on a copy where
     the form does not depend on B) and the geometry keys the row is there for; row_geometry() evaluates them with the tables' own
     restatements of the host rules, so a row that stops reaching its form fails on the CPU.
  2. POISONS: one non-finite value at a time, placed in the middle sample.
  3. case() / poisoned() / expected(): a row's clean inputs (x and gy rounded to the row's element type, held as fp32), the inputs under a
     poison, and what the reference's operators give for them: the families' autograd eager forms (one ATen op per reference line) in fp64
     on the CPU.  The staged oracles cannot serve here: they pick arg-max indices with one_hot, which has no index for a NaN."""
from collections import namedtuple
from types import SimpleNamespace

import torch

import spade_oracle as SO
import spade_plan as SP
from cbam_nchw_rows import NCHW_ROWS as CBAM_NCHW, cbam_nchw_geo, cbam_params
from conftest import synth
from eca_nchw_rows import NCHW_ROWS as ECA_NCHW, eca_params, nchw_geo as eca_nchw_geo
from head_nchw_rows import HEAD_NCHW_ROWS, head_geo, head_module, params_of, row_inputs
from oracle import maskcbam_oracle as O
from oracle import maskeca_oracle as E
from oracle import maskhead_oracle as HO

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NAN, INF = float("nan"), float("inf")
FAMILIES = ("cbam", "eca", "spade", "head")

# The channels-last tables of tests/test_gpu_channels_last_edges.py and tests/test_gpu_eca_channels_last.py are GPU test modules (their
# import marks everything gpu); the rows taken from them are restated here and test_nonfinite_host.py holds the restatement to the tables.
# name: (B, C, H, W, k, mask kind, 3-D mask)
CBAM_NHWC = {"v1_nj3_fold": (3, 130, 23, 17, 3, "mixed", False), "w3_cs4": (5, 12, 700, 3, 5, "all_negative", False),
             "v8_nj2_fold": (2, 520, 12, 12, 1, "none", False), "prob_f32": (9, 20, 37, 41, 15, "prob", False)}
ECA_NHWC = {"v1_nj3_fold": (3, 130, 23, 17, 3, "mixed", False), "w3_cs4": (5, 12, 700, 3, 5, "all_negative", False),
            "v8_nj2_fold": (2, 520, 12, 12, 1, "none", False), "prob_f32": (9, 20, 37, 41, 15, "prob", False)}

Row = namedtuple("Row", "family layout name B dtypes form what")


def R(family, layout, name, B, dtypes, what, **form):
    return Row(family, layout, name, B, tuple(dtypes.split()), form, what)


# form: geometry keys (the tables' own names) -> the value the row is there for; a dict value is per element type
ROWS = [
    # ---- MaskCBAM, NCHW (tests/cbam_nchw_rows.py) --------------------------------------------------------------------------------------
    R("cbam", "nchw", "v1_tx64_c130", 3, "f32 f16", "three-launch forward, staged MLP, unfolded backward, no projection planes",
      gate=False, fold=False, merge=False, stream=False, make_proj=0),
    R("cbam", "nchw", "v1_gate_k5", 3, "f32 f16 bf16", "fused gate launch, folded but unmerged backward, narrow planes at vec 1",
      gate=True, fold=True, merge=False, make_proj={"f32": 1, "f16": 0, "bf16": 0}),
    R("cbam", "nchw", "one_tile_merged", 3, "f32 f16", "fused gate launch, streamed MLP in the role workgroups, merged backward, narrow planes",
      gate=True, merge=True, stream=True, split_mlp=False, pool_ca=False, make_proj={"f32": 1, "f16": 0}, nox={"f32": True, "f16": False}),
    R("cbam", "nchw", "pool_ca_b1", 3, "f32", "k_pool's last arriver forms ca", pool_ca=True, gate=True, merge=True, make_proj=1),
    R("cbam", "nchw", "f16_gvec8_pool_ca", 3, "f16", "k_pool's last arriver forms ca, 16-byte k_gate lanes", pool_ca=True, gate=True, gvec=8),
    R("cbam", "nchw", "w1_hidden_eq_c", 3, "f32 f16", "split MLP, chunked hidden partials", split_mlp=True, pool_ca=False, merge=True,
      chunked_pgh=True),
    R("cbam", "nchw", "mfma_h16", 4, "f32 f16", "wide (MFMA) projection planes", merge=True, make_proj={"f32": 2, "f16": 0}),
    R("cbam", "nchw", "nomask_k9", 3, "f32 f16", "no mask; folded, unmerged backward at k = 9", stream=False, fold=True, merge=False),
    R("cbam", "nchw", "last_lane_prob", 3, "f32 f16", "raw-probability mask: an infinite mask value is not absorbed", merge=True,
      make_proj={"f32": 1, "f16": 0}),
    # ---- MaskCBAM, channels_last (tests/test_gpu_channels_last_edges.py) -----------------------------------------------------------
    R("cbam", "nhwc", "v1_nj3_fold", 3, "f32 f16 bf16", "lanes of one channel, three channel passes, partial fold block", vec=1, nj=3,
      fold_partial=True),
    R("cbam", "nhwc", "w3_cs4", 5, "f32 f16", "lanes of four channels, four lanes per pixel, two tiles", vec=4, cs=4, ntile=5),
    R("cbam", "nhwc", "v8_nj2_fold", 3, "f32 f16", "no mask; lanes of eight channels in half precision", vec={"f32": 4, "f16": 8},
      fold_partial=True),
    R("cbam", "nhwc", "prob_f32", 9, "f32 f16", "raw-probability mask", vec=4, cs=8),
    # ---- MaskECA, NCHW (tests/eca_nchw_rows.py): every row runs the role-workgroup backward ------------------------------------------
    R("eca", "nchw", "v1_tx64_c130", 3, "f32 f16 bf16", "vec 1, clamped channels, 3 tap roles", vec=1, tx=64, cpb=4, crem=2),
    R("eca", "nchw", "k_gt_c_b11", 11, "f32 f16", "all 15 tap roles and the dbeta role, taps wider than the channel axis", vec=1, ty=4),
    R("eca", "nchw", "w3_ty4", 5, "f32 f16", "vec 4, one pass of the channel loop", vec=4, ctx=64, ty=4),
    R("eca", "nchw", "nomask_k1", 3, "f32 f16", "no mask, k = 1", vec=4, tx=8, crem=8),
    R("eca", "nchw", "v1_tx256_prob", 9, "f32 f16", "raw-probability mask", vec=1, tx=256),
    # ---- MaskECA, channels_last (tests/test_gpu_eca_channels_last.py) -----------------------------------------------------------------
    R("eca", "nhwc", "v1_nj3_fold", 3, "f32 f16 bf16", "lanes of one channel, three channel passes, partial fold block", vec=1, nj=3,
      fold_partial=True),
    R("eca", "nhwc", "w3_cs4", 5, "f32 f16", "lanes of four channels, four lanes per pixel", vec=4, cs=4),
    R("eca", "nhwc", "v8_nj2_fold", 3, "f32 f16", "no mask; lanes of eight channels in half precision", vec={"f32": 4, "f16": 8},
      fold_partial=True),
    R("eca", "nhwc", "prob_f32", 9, "f32 f16", "raw-probability mask", vec=4, cs=8),
    # ---- MGAMaskHead (tests/head_nchw_rows.py), each row in training and in eval mode; the channels-last kernels run the same rows ----
    R("head", "nchw", "v1_guard", 3, "f32 f16 bf16", "vec 1; fp32 MFMAs in fp32, half MFMAs in half (16-byte weight form)", vec=1,
      fw_w="guard", gw2=0),
    R("head", "nchw", "gather_c6", 3, "f32 f16", "the gather form of the weights: fp32 MFMAs in every element type", vec=1, fw_w="gather"),
    R("head", "nchw", "ksplit_c132", 3, "f32 f16", "vec 4, K split over four waves, the LDS-staged dW1", vec=4, fw_kw=4, gw2=1),
    R("head", "nhwc", "v1_guard", 3, "f32 f16 bf16", "four-channel lanes", c_lanes=4),
    R("head", "nhwc", "gather_c6", 3, "f32 f16", "per-element lanes along C", c_lanes=1),
    R("head", "nhwc", "ksplit_c132", 3, "f32 f16", "four-channel lanes, hidden 24", c_lanes=4),
    # ---- MaskSPADE (tests/spade_plan.py): hidden widths and channel tails; both layouts run every row ------------------------------
    R("spade", "both", (32, 16, 8), 3, "f32 f16 bf16", "hidden 16, one exact tile", hidden=16, tw=8, tiles=(1, 1), c16=False),
    R("spade", "both", (48, 30, 22), 3, "f32 f16", "batch norm, hidden 48, C % 32 == 16, ragged tiles", hidden=48, norm="bn", c16=True,
      ragged=(True, True), dh=(2, 16)),
    R("spade", "both", (80, 60, 10), 3, "f32 f16", "hidden 64, channel blocks 48 + 32, three dh rounds", hidden=64, fwd=(48, 2, 32),
      dh=(3, 16)),
    R("spade", "both", (32, 5, 3), 3, "f32 f16", "hidden 32, odd H*W", hidden=32, tiles=(1, 1)),
    R("spade", "both", (32, 5, 3), 3, "f32", "hidden 32, raw mask (use_sigmoid_mask off): an infinite mask value is not absorbed", hidden=32,
      use_sigmoid=False),
]
# MaskSPADE: the seeds of tests/spade_plan.py were searched at the table's B; at B = 3 (and with the absorbed mask values in place) these are
# the first seeds from the row's own for which no fp64 pre-activation has |pre| < 1e-5, so no ReLU branch can differ on the device
# (test_nonfinite_host.py re-checks it)
SPADE_SEEDS = {"spade-both-48x30x22": 209, "spade-both-80x60x10": 1351}


def row_id(r):
    name = r.name if isinstance(r.name, str) else "x".join(str(v) for v in r.name) + ("-raw" if r.form.get("use_sigmoid") is False else "")
    return f"{r.family}-{r.layout}-{name}"


def layouts(r):
    return ("nchw", "nhwc") if r.layout == "both" else (r.layout,)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. geometry
# ------------------------------------------------------------------------------------------------------------------------------------
def _table_row(table, name):
    (row,) = [t for t in table if t[0] == name]
    return row


def nhwc_vec(C, dt):
    """host.cuh's nhwc_vec as tests/test_abi_nhwc.py restates it"""
    return 8 if (dt != "f32" and C % 8 == 0) else (4 if C % 4 == 0 else 1)


def row_geometry(r, dt):
    """The launch form of row r at element type dt, with r.B samples, from the restatements the family's table is checked with."""
    if r.family == "cbam" and r.layout == "nchw":
        _, _, _, C, H, W, k, hidden, kind, _, mask_grad, _, _ = _table_row(CBAM_NCHW, r.name)
        return cbam_nchw_geo(r.B, C, H, W, k, hidden, dt, kind != "none" and mask_grad)
    if r.family == "eca" and r.layout == "nchw":
        _, _, _, C, H, W, *_ = _table_row(ECA_NCHW, r.name)
        return eca_nchw_geo(r.B, C, H, W)
    if r.family in ("cbam", "eca"):
        from test_abi_nhwc import _nhwc_geo
        _, C, H, W, *_ = (CBAM_NHWC if r.family == "cbam" else ECA_NHWC)[r.name]
        return _nhwc_geo(C, H, W, nhwc_vec(C, dt))
    if r.family == "head":
        _, _, _, C, hid, H, W, _, _ = _table_row(HEAD_NCHW_ROWS, r.name)
        g = head_geo(r.B, C, hid, H, W)
        g["c_lanes"] = nhwc_vec(C, dt) if r.layout == "nhwc" else None
        return g
    c = spade_case(r)
    g = SP.plan_of(c._replace(B=r.B))
    g.update(hidden=c.hidden, norm=c.norm, use_sigmoid=r.form.get("use_sigmoid", True))
    return g


def form_of(r, dt):
    return {k: (v[dt] if isinstance(v, dict) else v) for k, v in r.form.items()}


def spade_case(r):
    (c,) = [c for c in SP.CASES if (c.C, c.H, c.W) == tuple(r.name)]
    return c


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. poisons
# ------------------------------------------------------------------------------------------------------------------------------------
Poison = namedtuple("Poison", "id target value")
POISONS = [Poison("x_nan", "x", NAN), Poison("x_pinf", "x", INF), Poison("x_ninf", "x", -INF),
           Poison("mask_nan", "mask", NAN), Poison("mask_pinf", "mask", INF), Poison("mask_ninf", "mask", -INF),
           Poison("gy_nan", "gy", NAN), Poison("gy_pinf", "gy", INF), Poison("param_nan", "param", NAN)]
# the parameter element that is poisoned: MaskCBAM one weight of the shared MLP's first layer, MaskECA the centre tap, the mask head one weight
# of the 1x1 projection, MaskSPADE one centre tap of conv_gamma (a single output channel)
PARAM_TARGET = {"cbam": "w1", "eca": "w", "head": "w1", "spade": "conv_gamma.weight"}


def poisons_of(case):
    return [p for p in POISONS if p.target != "mask" or case.inp["mask"] is not None]


def absorbed(case, p):
    """An infinite mask logit under use_sigmoid: the sigmoid saturates to exactly 0 or 1 and the reference stays finite everywhere."""
    return p.target == "mask" and p.value in (INF, -INF) and case.use_sig


def middle(t, b):
    """the element of sample b a poison goes to: the middle of every further axis"""
    return (b,) + tuple(n // 2 for n in t.shape[1:])


def poisoned(case, p):
    """-> a copy of case.inp with the poison in place (the middle sample; a parameter: its middle element)"""
    inp = dict(case.inp)
    if p.target == "param":
        params = dict(inp["params"])
        t = params[PARAM_TARGET[case.family]].clone()
        t[tuple(n // 2 for n in t.shape)] = p.value
        params[PARAM_TARGET[case.family]] = t
        inp["params"] = params
    else:
        t = inp[p.target].clone()
        t[middle(t, case.B // 2)] = p.value
        inp[p.target] = t
    return inp


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. cases and what the reference's operators give
# ------------------------------------------------------------------------------------------------------------------------------------
CBAM_KEYS = ("w1", "b1", "w2", "b2", "wsa", "beta")
HEAD_KEYS = ("w1", "gamma", "beta", "wh", "bh")
_cases, _expected = {}, {}


def _rounded(t, dt):
    return t.to(DT[dt]).float()


def case(r, dt, training=True):
    """-> the row's clean inputs: inp = dict(x, mask | None, gy, params {name: fp32 tensor}[, running (mean, var)]) and its configuration.
    Computed once per (row, dtype, mode) and shared: the tensors must not be written to."""
    key = (row_id(r), dt, training)
    if key in _cases:
        return _cases[key]
    c = SimpleNamespace(row=r, family=r.family, dt=dt, dtype=DT[dt], B=r.B, training=training, use_sig=True, cfg={})
    if r.family in ("cbam", "eca"):
        if r.layout == "nchw":
            row = _table_row(CBAM_NCHW if r.family == "cbam" else ECA_NCHW, r.name)
            C, H, W, k = row[3:7]
            kind, mask3d, tiny_thr = (row[8], row[9], row[11]) if r.family == "cbam" else (row[7], row[8], row[10])
            hidden = row[7] if r.family == "cbam" else None
        else:
            _, C, H, W, k, kind, mask3d = (CBAM_NHWC if r.family == "cbam" else ECA_NHWC)[r.name]
            tiny_thr, hidden = 1e-4, None
        x, mask, gy = synth(r.B, C, H, W, seed=300 + C + H, mask_kind=kind, mask3d=mask3d)
        c.use_sig = kind != "prob"
        if r.family == "cbam":
            p = cbam_params(C, k, hidden, seed=C) if hidden is not None else _nhwc_cbam_params(C, k, seed=C)
            params = dict(zip(CBAM_KEYS, (p.w1, p.b1, p.w2, p.b2, p.wsa, p.beta)))
            c.cfg = dict(hidden=p.w1.shape[0], k=k, use_sigmoid_mask=c.use_sig, tiny_thr=tiny_thr, eps=1e-6)
        else:
            p = eca_params(k, seed=C)
            params = dict(w=p.w, beta=p.beta)
            c.cfg = dict(k=k, use_sigmoid_mask=c.use_sig, tiny_thr=tiny_thr, eps=1e-6)
        c.inp = dict(x=_rounded(x, dt), mask=mask, gy=_rounded(gy, dt), params=params)
    elif r.family == "head":
        _, _, _, C, hid, H, W, _, _ = _table_row(HEAD_NCHW_ROWS, r.name)
        m = head_module(C, hid, seed=1000 + C + hid, training=training)
        x, gl = row_inputs(r.B, C, H, W, dt, 2000 + 7 * C + H)
        p = params_of(m)
        c.inp = dict(x=x, mask=None, gy=gl, params=dict(zip(HEAD_KEYS, (p.w1, p.gamma, p.beta, p.wh, p.bh))),
                     running=(p.running_mean, p.running_var))
        c.cfg = dict(eps=p.eps, momentum=p.momentum, training=training, hid=hid)
    else:
        from test_gpu_spade import live_case                    # (the module's import needs no GPU)
        sc = spade_case(r)
        c.use_sig = r.form.get("use_sigmoid", True)
        m, x, mask, gy = live_case(r.B, sc.C, sc.H, sc.W, sc.norm, seed=SPADE_SEEDS.get(row_id(r), sc.seed), hidden=sc.hidden)
        params = {k: v.detach().clone() for k, v in m.state_dict().items() if k in SO.PARAM_KEYS}
        c.inp = dict(x=_rounded(x, dt), mask=mask, gy=_rounded(gy, dt), params=params)
        if sc.norm == "bn":
            c.inp["running"] = (m.norm.running_mean.detach().clone(), m.norm.running_var.detach().clone())
        c.cfg = dict(hidden=sc.hidden, norm_type=sc.norm, use_sigmoid_mask=c.use_sig, eps=sc.eps, momentum=sc.momentum, training=True)
    _cases[key] = c
    return c


def _nhwc_cbam_params(C, k, seed):
    """test_gpu_channels_last_edges._params"""
    p = O.Params.default_init(C, k=k, seed=seed)
    with torch.no_grad():
        for t in (p.w1, p.b1, p.w2, p.b2):
            t.add_(0.3 * torch.randn(t.shape, generator=torch.Generator().manual_seed(seed)))
        p.wsa.mul_(3.0)
        p.beta.fill_(0.4)
    return p


def eager_step(c, inp, dtype=torch.float64):
    """One forward + backward of the family's autograd eager form on inp, in `dtype` -> {output name: tensor}: y, gx, gmask (masked rows), g.<parameter>
    for every parameter, running_mean / running_var where the block keeps batch statistics."""
    d = lambda t: None if t is None else t.to(dtype)
    x, mask, gy, P = d(inp["x"]), d(inp["mask"]), d(inp["gy"]), {k: d(v) for k, v in inp["params"].items()}
    if c.family == "cbam":
        cfg = O.Config(use_sigmoid_mask=c.cfg["use_sigmoid_mask"], tiny_thr=c.cfg["tiny_thr"], eps=c.cfg["eps"])
        y, g = O.reference_form_step(x, mask, O.Params(*(P[k] for k in CBAM_KEYS)), cfg, gy)
        out = dict(y=y, gx=g["gx"], gmask=g["gmask"], **{"g." + k: g["g" + k] for k in CBAM_KEYS})
    elif c.family == "eca":
        cfg = E.EcaConfig(use_sigmoid_mask=c.cfg["use_sigmoid_mask"], tiny_thr=c.cfg["tiny_thr"], eps=c.cfg["eps"])
        y, g = E.reference_form_step(x, mask, E.EcaParams(P["w"], P["beta"]), cfg, gy)
        out = dict(y=y, gx=g["gx"], gmask=g["gmask"], **{"g.w": g["gw"], "g.beta": g["gbeta"]})
    elif c.family == "head":
        rm, rv = (d(t) for t in inp["running"])
        p = HO.HeadParams(P["w1"], P["gamma"], P["beta"], rm, rv, P["wh"], P["bh"], c.cfg["eps"], c.cfg["momentum"])
        y, g = HO.reference_form_all(x, p, gy, c.cfg["training"])
        out = dict(y=y, gx=g["gx"], gmask=None, running_mean=g["running_mean"], running_var=g["running_var"],
                   **{"g." + k: g["g" + k] for k in HEAD_KEYS})
    else:
        run = None if "running" not in inp else tuple(d(t) for t in inp["running"])
        y, g = SO.reference_form_step(x, mask, P, gy, c.cfg["norm_type"], True, c.cfg["use_sigmoid_mask"], c.cfg["eps"], run, c.cfg["momentum"])
        out = dict(y=y, gx=g["gx"], gmask=g["gmask"], **{"g." + k: g[k] for k in SO.PARAM_KEYS})
        if run is not None:
            out.update(running_mean=g["running_mean"], running_var=g["running_var"])
    return {k: v for k, v in out.items() if v is not None}


def expected(c, p=None):
    """What the reference's operators give for the case under poison p (None: clean), in fp64; computed once and shared."""
    key = (row_id(c.row), c.dt, c.training, None if p is None else p.id)
    if key not in _expected:
        _expected[key] = eager_step(c, c.inp if p is None else poisoned(c, p))
    return _expected[key]


FEATURE_OUTPUTS = ("y", "gx", "gmask")


def is_param_output(name):
    return name.startswith("g.") or name.startswith("running_")


def cbam_near_tie_pixels(c, inp):
    """(B, H*W) pixels whose channel arg-max is decided by < 1e-6 relative (cbam_nchw_rows.near_tie_pixels), from the staged fp64 oracle's
    forward on inp where that is finite, else on the clean inputs (the samples a poison leaves alone have the clean forward)."""
    from cbam_nchw_rows import near_tie_pixels
    cfg = O.Config(use_sigmoid_mask=c.cfg["use_sigmoid_mask"], tiny_thr=c.cfg["tiny_thr"], eps=c.cfg["eps"])
    for cand in (inp, c.inp):
        m = None if cand["mask"] is None else cand["mask"].double()
        y, ctx = O.forward(cand["x"].double(), m, O.Params(*(cand["params"][k] for k in CBAM_KEYS)).to(torch.float64), cfg)
        if bool(torch.isfinite(y).all()):
            return near_tie_pixels(cand["x"], ctx)
    raise AssertionError("the clean inputs give a finite forward")
