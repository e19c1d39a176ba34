"""fp64 statement of the detection criterion (include/mgadet.h) for the tests, with the magnitudes the error bars are made of.

Written ground truth by ground truth and anchor by anchor where the library's host path (mga_yolo_amd/detloss.py) is vectorised, so the
two share no code; gradients come from autograd on the fp64 graph, one backward per loss component.

Bars: |err| <= K * eps_dtype * terms, per quantity.  A target score is  metric_a * pos_overlap_g / pos_metric_g  with
metric = score^0.5 * overlap^6 and overlap = CIoU = iou - rho2 / c2 - v alpha, a difference: rounding reaches the overlap relative to
T = |iou| + |rho2 / c2| + |v alpha|, not to the overlap itself, and the sixth power carries it six times.  So an assigned anchor has
  amp_a            = 1 + 6 T_a / ov_a + 6 T_m / ov_m + T_o / ov_o   (m, o: the anchors that give its ground truth's largest metric and overlap)
and, with amp = 1 for background anchors and amp_tss = sum(score * amp) / sum(score) where tss is that sum (1 where tss is clamped to 1):
  target_scores    terms = score * amp_a (where the fp64 score is exactly 0 the result must be exactly 0)
  loss[i]          terms = gain_i * B / tss * amp_tss * sum_a |contribution_a| * amp_a
  dL/dfeats        terms = amp_a * amp_tss * sum_i |up_i| * m_i, m_i the component's gradient magnitude: for a class channel
                   |f| (sigmoid + target); for a bin channel the LARGEST |gradient| among its side's 16 bins (a side's gradients sum
                   to zero: their common scale, not each bin's own value, is what rounding is relative to)
"""
import json
import math
import os

import numpy as np
import torch

REG = 16
EPS = 1e-7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# per quantity, twice the largest ratio of the reference's own fp32 run against its fp64 run over the committed cases
# (tools/gen_golden_det.py measured them into det_ratios.json): the kernels sum in another order than torch does
K = {}
if os.path.exists(os.path.join(GOLDEN, "det_ratios.json")):          # absent only while the generator writes the fixtures for the first time
    with open(os.path.join(GOLDEN, "det_ratios.json")) as _f:
        _WORST = json.load(_f)["worst"]
    K = dict(loss=2 * _WORST["loss"], target_scores=2 * _WORST["target_scores"], grad=2 * max(_WORST["g1"], _WORST["gnu"]))
CASES = ("b2_64_nc1", "b2_64_nc3", "b3_96x64_nc5", "b2_128_nc2", "ties", "empty")


def load_case(name):
    z = np.load(os.path.join(GOLDEN, f"det_{name}.npz"))
    c = {k: z[k] for k in z.files}
    c["feats"] = [torch.from_numpy(c[f"feat{l}"]) for l in range(len(c["strides"]))]
    c["labels"] = tuple(torch.from_numpy(c[k]) for k in ("batch_idx", "cls", "bboxes"))
    c["kw"] = dict(nc=int(c["nc"]), strides=tuple(int(s) for s in c["strides"]), gains=tuple(float(g) for g in c["gains"]), topk=int(c["topk"]))
    return c


def ciou(p, q, parts=False):
    """parts: also |iou| + |rho2 / c2| + |v alpha|, what the difference is formed from"""
    w1, h1, w2, h2 = p[..., 2] - p[..., 0], p[..., 3] - p[..., 1] + EPS, q[..., 2] - q[..., 0], q[..., 3] - q[..., 1] + EPS
    iw = (torch.minimum(p[..., 2], q[..., 2]) - torch.maximum(p[..., 0], q[..., 0])).clamp(min=0)
    ih = (torch.minimum(p[..., 3], q[..., 3]) - torch.maximum(p[..., 1], q[..., 1])).clamp(min=0)
    inter = iw * ih
    iou = inter / (w1 * h1 + w2 * h2 - inter + EPS)
    cw = torch.maximum(p[..., 2], q[..., 2]) - torch.minimum(p[..., 0], q[..., 0])
    ch = torch.maximum(p[..., 3], q[..., 3]) - torch.minimum(p[..., 1], q[..., 1])
    rho2 = ((q[..., 0] + q[..., 2] - p[..., 0] - p[..., 2]) ** 2 + (q[..., 1] + q[..., 3] - p[..., 1] - p[..., 3]) ** 2) / 4
    v = 4 / math.pi ** 2 * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = (v / (v - iou + 1 + EPS)).detach()
    far = rho2 / (cw ** 2 + ch ** 2 + EPS)
    val = iou - (far + v * alpha)
    return (val, (iou.abs() + far.abs() + (v * alpha).abs()).detach()) if parts else val


def oracle(feats, batch_idx, cls, bboxes, *, nc, strides=(8, 16, 32), gains=(7.5, 0.5, 1.5), topk=10, lowest_first=True):
    """feats: fp64 leaves or plain tensors (B, 64 + nc, H_l, W_l).  Returns loss, items, fg, target_gt (label row), target_scores,
    target_bboxes (pixels), weight, comp_grads (per component, per level), terms and picks."""
    f64 = torch.float64
    xs = [f.detach().to(f64).clone().requires_grad_(True) for f in feats]
    B = xs[0].shape[0]
    no = 4 * REG + nc
    x = torch.cat([f.reshape(B, no, -1) for f in xs], 2).permute(0, 2, 1)
    A = x.shape[1]
    anc, st = [], []
    for f, s in zip(xs, strides):
        for yy in range(f.shape[2]):
            for xx in range(f.shape[3]):
                anc.append((xx + 0.5, yy + 0.5)); st.append(float(s))
    anc, st = torch.tensor(anc, dtype=f64), torch.tensor(st, dtype=f64)[:, None]
    dist, scores = x[..., :4 * REG].reshape(B, A, 4, REG), x[..., 4 * REG:]
    d = (dist.softmax(-1) * torch.arange(REG, dtype=f64)).sum(-1)
    pred = torch.cat((anc - d[..., :2], anc + d[..., 2:]), -1)
    img_w, img_h = xs[0].shape[3] * strides[0], xs[0].shape[2] * strides[0]
    bidx, cl, bb = batch_idx.to(f64), cls.to(f64), bboxes.to(f64).reshape(-1, 4)
    fg = torch.zeros(B, A, dtype=torch.bool)
    t_row = torch.full((B, A), -1, dtype=torch.int64)
    norm = torch.zeros(B, A, dtype=f64)
    t_box = torch.zeros(B, A, 4, dtype=f64)
    t_lab = torch.zeros(B, A, dtype=torch.int64)
    amp = torch.ones(B, A, dtype=f64)
    pp, ap, sg = (pred * st).detach(), anc * st, scores.detach().sigmoid()
    picks = {}                                                   # per labelled image: its rows, the top-k picks before the contest, the metrics
    for b in range(B):
        rows = [r for r in range(bidx.numel()) if int(bidx[r]) == b]
        if not rows:
            continue
        M = len(rows)
        gt = torch.stack([torch.stack((bb[r, 0] * img_w - bb[r, 2] * img_w / 2, bb[r, 1] * img_h - bb[r, 3] * img_h / 2,
                                       bb[r, 0] * img_w + bb[r, 2] * img_w / 2, bb[r, 1] * img_h + bb[r, 3] * img_h / 2)) for r in rows])
        gt = gt.float().double()                                 # the reference's xywh2xyxy writes into an fp32 tensor whatever its input's type
        lab = [min(max(int(cl[r]), 0), nc - 1) for r in rows]
        ov, met, cond = torch.zeros(M, A, dtype=f64), torch.zeros(M, A, dtype=f64), torch.zeros(M, A, dtype=f64)
        cand, pos = torch.zeros(M, A, dtype=torch.bool), torch.zeros(M, A, dtype=torch.bool)
        for g in range(M):
            if not gt[g].sum() > 0:
                continue
            delta = torch.stack((ap[:, 0] - gt[g, 0], ap[:, 1] - gt[g, 1], gt[g, 2] - ap[:, 0], gt[g, 3] - ap[:, 1]), -1).amin(-1)
            cand[g] = delta > 1e-9
            val, mag = ciou(gt[g][None], pp[b], parts=True)
            ov[g] = val.clamp(min=0) * cand[g]
            cond[g] = torch.where(ov[g] > 0, mag / ov[g].clamp(min=1e-300), torch.zeros((), dtype=f64))
            met[g] = sg[b, :, lab[g]].sqrt() * ov[g] ** 6
            inside = [a for a in range(A) if cand[g, a]]
            inside.sort(key=lambda a: (-float(met[g, a]), a if lowest_first else -a))
            for a in inside[:topk]:
                pos[g, a] = True
        picks[b] = (rows, pos.clone(), met.clone())
        for a in range(A):
            if pos[:, a].sum() > 1:
                win = int(ov[:, a].argmax())                     # first index on a tie
                pos[:, a] = False
                pos[win, a] = True
        for g in range(M):
            if not pos[g].any():
                continue
            pm, po = (met[g] * pos[g]).max(), (ov[g] * pos[g]).max()
            am, ao = int((met[g] * pos[g]).argmax()), int((ov[g] * pos[g]).argmax())
            for a in torch.nonzero(pos[g]).flatten().tolist():
                fg[b, a], t_row[b, a], t_box[b, a], t_lab[b, a] = True, rows[g], gt[g], lab[g]
                norm[b, a] = met[g, a] * po / (pm + 1e-9)
                amp[b, a] = 1 + 6 * cond[g, a] + 6 * cond[g, am] + cond[g, ao]
    t_scores = torch.nn.functional.one_hot(t_lab, nc).to(f64) * norm[..., None]
    tss = t_scores.sum().clamp(min=1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(scores, t_scores, reduction="none")
    w = norm[fg]
    tb = (t_box / st)[fg]
    box_a = (1 - ciou(pred[fg], tb)) * w
    a_fg = anc[None].expand(B, -1, -1)[fg]
    ltrb = torch.cat((a_fg - tb[:, :2], tb[:, 2:] - a_fg), -1).clamp(0, REG - 1 - 0.01)
    tl = ltrb.long()
    wl = (tl + 1).to(f64) - ltrb
    logp = dist[fg].log_softmax(-1)
    ce = -(logp.gather(-1, tl[..., None]).squeeze(-1) * wl + logp.gather(-1, tl[..., None] + 1).squeeze(-1) * (1 - wl))
    dfl_a = ce.mean(-1) * w
    gn = torch.tensor([float(g) for g in gains], dtype=f64)
    comp = torch.stack((box_a.sum(), bce.sum(), dfl_a.sum())) / tss
    loss = comp * gn * B
    comp_grads = []
    for i in range(3):
        gs = torch.autograd.grad(loss[i], xs, retain_graph=True, allow_unused=True)
        comp_grads.append([torch.zeros_like(x_) if g_ is None else g_ for g_, x_ in zip(gs, xs)])
    # ---- magnitudes
    amp_tss = float((norm * amp).sum() / norm.sum()) if float(norm.sum()) >= 1 else 1.0
    terms = dict(loss=(torch.stack(((box_a.abs() * amp[fg]).sum(), (bce.abs().sum(-1) * amp).sum(), (dfl_a.abs() * amp[fg]).sum()))
                       / tss * amp_tss * gn.abs() * B).detach(),
                 target_scores=(t_scores.detach().abs() * amp[..., None]), amp=amp, amp_tss=amp_tss)
    f_cls = float(gn[1].abs() * B / tss)
    mags = []                                                    # per component, per level
    for i in range(3):
        lv = []
        for l, g_ in enumerate(comp_grads[i]):
            Bq, _, H, W = g_.shape
            m = torch.zeros_like(g_)
            o = sum(f.shape[2] * f.shape[3] for f in xs[:l])
            if i == 1:
                ts = t_scores[:, o:o + H * W].permute(0, 2, 1).reshape(Bq, nc, H, W)
                m[:, 4 * REG:] = f_cls * (xs[l][:, 4 * REG:].detach().sigmoid() + ts)
            else:
                side = g_[:, :4 * REG].abs().reshape(Bq, 4, REG, H, W).amax(2, keepdim=True).expand(-1, -1, REG, -1, -1)
                m[:, :4 * REG] = side.reshape(Bq, 4 * REG, H, W)
            lv.append(m * amp[:, o:o + H * W].reshape(Bq, 1, H, W) * amp_tss)
        mags.append(lv)
    terms["grad_mags"] = mags
    return dict(loss=loss.detach(), items=(comp * gn).detach(), fg=fg, target_gt=t_row, target_scores=t_scores.detach(),
                target_bboxes=t_box, weight=norm, comp_grads=comp_grads, terms=terms, tss=float(tss), picks=picks)


def grads(o, level, upstream):
    """dL/dfeats[level] for the upstream vector, from the component gradients of oracle()."""
    return sum(float(u) * o["comp_grads"][i][level] for i, u in enumerate(upstream))


def grad_terms(terms, level, upstream):
    return sum(abs(float(u)) * terms["grad_mags"][i][level] for i, u in enumerate(upstream))


def check(name, got, want, terms, eps, k):
    """|got - want| <= k * eps * terms element-wise, exact where terms == 0; returns the largest ratio (for the figures), asserts the bar."""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    terms = torch.as_tensor(terms).double().cpu().expand_as(want)
    err = (got - want).abs()
    zero = terms == 0
    assert torch.equal(got[zero], want[zero]), f"{name}: must be exact where its terms are 0"
    ratio = float((err[~zero] / (eps * terms[~zero])).max()) if (~zero).any() else 0.0
    print(f"{name}: max |err| / (eps * terms) = {ratio:.2f} (bar {k})")
    assert ratio <= k, f"{name}: {ratio:.2f} > {k}"
    return ratio
