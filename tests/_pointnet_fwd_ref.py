"""Plain torch restatement (CPU; the tests use float64) of the trunk of the PointNet forward, layer by layer, with the bound
each layer's fp32 evaluation is held to.  No project code.  tests/test_pointnet_fwd_ref.py pins it to the oracle's forward.

    p = T3^T x                        (Model/PointNet.py:138; p = x without T3)
    h = relu(w1 p + b1)               the folded first layer, 64 rows
    y = relu(W[b] h + bias)           a stage: 64 inputs, 64 or 128 outputs, shared or per-instance weights
    gate = pre > 0                    pre = the value before the relu

Bound (tests/test_gpu_pointnet_bwd.py, "as for the forward kernels"): |got - ref| <= 4 sqrt(n) 2^-24 mag + 2^-22 |ref|, n =
the terms of the longest sum behind an entry, mag = the float64 sum of the absolute values of the products (and the bias).

  * A stage: n = 65 (64 products and the bias), mag = |W| |h| + |bias|, PLUS |W| (bound of its input): the kernel evaluates
    the stage on its own, already rounded input, and the relu in between is 1-Lipschitz, so an input error e reaches pre as at
    most |W| e.  (The own term is stated on the exact input's magnitude; the rounded input's differs from it by the input's
    bound, a second-order term the factor 4 has room for.)
  * The first layer is the ONE fp32 expression pn_first_layer, w.x p0 + w.y p1 + w.z p2 + w.w behind p_c = x0 T[0][c] + x1
    T[3+c] + x2 T[6+c], fused or not.  With u = 2^-24 and scale = |w1| (|T3|^T |x|) + |b1|: p carries at most 3 u |T3|^T |x| (a
    three-term sum), the outer expression at most 4 u scale on top (three products, three adds), 7 u scale in all (4 u scale
    without T3), to first order.  Stated in the common form with n = the terms of the nested sum -- 3 x 3 + 1 = 10 with T3
    (4 sqrt(10) u = 12.6 u), 3 + 1 = 4 without (8 u) -- it covers both.

Every function returns what a test needs of a layer: y, pre, bound (of pre, hence of y), mag.  The keyword arguments named
drop_* / wrong_* / *_transposed / gate_before_bias restate a DEFECTIVE kernel; the sensitivity tests use them to show that
the bound of a case would notice.
"""
from __future__ import annotations

import torch

from tests._pointnet_bwd_ref import pack_gate_bits, tolerance, worst_ratio  # noqa: F401  (re-exported for the tests)

STAGE_TERMS = 65


def unpack_gate_bits(words, N):
    """int64 words [B, ceil(N/64), C] -> bool [B, C, N]; the bits of columns >= N are dropped (the header leaves them open)"""
    B, T, C = words.shape
    sh = torch.arange(64, dtype=torch.int64)
    bits = ((words.cpu().unsqueeze(-1) >> sh) & 1).bool()             # [B, T, C, 64]
    return bits.permute(0, 2, 1, 3).reshape(B, C, T * 64)[:, :, :N].contiguous()


def first_layer(x3, w1, b1, T3=None, T3_transposed=False, drop_term=None):
    """-> dict(y, pre, bound, mag) of h = relu(w1 (T3^T x3) + b1): x3 [B,3,N], w1 [64,3], b1 [64], T3 [B,3,3] or None.
    T3_transposed: p = T3 x (the defect); drop_term: coordinate c of p left out of the sum."""
    if T3 is None:
        p, pa, n = x3, x3.abs(), 4
    else:
        eq = "bcd,bdn->bcn" if T3_transposed else "bdc,bdn->bcn"
        p, pa, n = torch.einsum(eq, T3, x3), torch.einsum(eq, T3.abs(), x3.abs()), 10
    w = w1
    if drop_term is not None:
        w = w1.clone()
        w[:, drop_term] = 0
    pre = torch.einsum("kc,bcn->bkn", w, p) + b1.view(1, -1, 1)
    mag = torch.einsum("kc,bcn->bkn", w1.abs(), pa) + b1.abs().view(1, -1, 1)
    return {"y": pre.clamp_min(0), "pre": pre, "bound": tolerance(pre, mag, n), "mag": mag}


def stage(h, W, bias, bound_in=None, drop_term=None, wrong_bias=None, instance0_weights=False, gate_before_bias=False):
    """-> dict(y, pre, bound, mag, gate) of y = relu(W[b] h + bias): h [B,64,N], W [Co,64] or [B,Co,64], bias [Co]; bound_in =
    the bound h is held to (None: h is exact).  Defects: drop_term = input row k left out; wrong_bias = another bias vector
    used; instance0_weights = W[0] for every instance; gate_before_bias = the gate is taken on W h."""
    B = h.shape[0]
    Wb = W if W.dim() == 3 else W.unsqueeze(0).expand(B, -1, -1)
    Wuse = Wb[:1].expand(B, -1, -1) if instance0_weights else Wb
    hu = h
    if drop_term is not None:
        hu = h.clone()
        hu[:, drop_term] = 0
    acc = torch.einsum("bok,bkn->bon", Wuse, hu)
    pre = acc + (bias if wrong_bias is None else wrong_bias).view(1, -1, 1)
    mag = torch.einsum("bok,bkn->bon", Wb.abs(), h.abs()) + bias.abs().view(1, -1, 1)
    bound = tolerance(pre, mag, STAGE_TERMS)
    if bound_in is not None:
        bound = bound + torch.einsum("bok,bkn->bon", Wb.abs(), bound_in)
    return {"y": pre.clamp_min(0), "pre": pre, "bound": bound, "mag": mag, "gate": (acc if gate_before_bias else pre) > 0}


def chain(stages, X=None, cloud=None, defect=None):
    """A chain of 1, 2 or 3 stages behind X [B,64,N] (exact) or behind the first layer of cloud = (x3, T3 or None, w1, b1).
    stages: [(W, bias), ...].  defect: (stage index or "first", keyword dict) handed to that layer.
    -> (layers, first): one dict per stage, and the first layer's dict or None."""
    first = None
    if cloud is not None:
        x3, T3, w1, b1 = cloud
        first = first_layer(x3, w1, b1, T3, **(defect[1] if defect and defect[0] == "first" else {}))
        first["gate"] = first["pre"] > 0
        h, bound = first["y"], first["bound"]
    else:
        h, bound = X, None
    layers = []
    for i, (W, bias) in enumerate(stages):
        L = stage(h, W, bias, bound, **(defect[1] if defect and defect[0] == i else {}))
        layers.append(L)
        h, bound = L["y"], L["bound"]
    return layers, first


def undecided(layer):
    """bool: the entries whose gate the bound leaves open (|pre| within the bound of zero)"""
    return layer["pre"].abs() <= layer["bound"]


def gate_ratio(bits, layer):
    """(wrong, open share): the number of decided entries whose bit is not the float64 gate, and the share left open"""
    und = undecided(layer)
    wrong = int(((bits != (layer["pre"] > 0)) & ~und).sum())
    return wrong, float(und.double().mean())


# ---------------------------------------------------------------------------------------------------------------------
# behind the trunk: the 1024-wide layers and the heads, for the comparison with the oracle's logits
# ---------------------------------------------------------------------------------------------------------------------
def wide_max(h, W, bias, taps):
    """relu(max_n conv(h) + bias): h [B,128,N], W [1024, taps*128] with k = tap*128 + ci (zero padded)"""
    w = W.view(1024, taps, 128).permute(0, 2, 1)
    return (torch.nn.functional.conv1d(h, w, padding=taps // 2).max(dim=2).values + bias).clamp_min(0)


def fc_head(f, t):
    """the three fully connected layers of a head; t: dict with f1 / fb1, f2 / fb2, f3 / fb3"""
    f = (f @ t["f1"].t() + t["fb1"]).clamp_min(0)
    f = (f @ t["f2"].t() + t["fb2"]).clamp_min(0)
    return f @ t["f3"].t() + t["fb3"]


def pointnet_trunk(packed, pc):
    """The whole forward from the folded weights (geoa3_amd.pointnet.pack_pointnet's dict, any dtype) composed of the
    functions above, in the order of geoa3_pointnet_forward.  -> dict of every intermediate and the logits."""
    B = pc.shape[0]
    t3, t64 = packed["t3"], packed["t64"]
    out = {}
    (a2,), _ = chain([(t3["w2"], t3["b2"])], cloud=(pc, None, t3["w1"], t3["b1"]))
    out["a2"] = a2
    out["T3"] = fc_head(wide_max(a2["y"], t3["w3"], t3["b3"], 1), t3).view(B, 3, 3)
    (h2, c1, c2), h1 = chain([(packed["w2"], packed["b2"]), (t64["w1"], t64["b1"]), (t64["w2"], t64["b2"])],
                             cloud=(pc, out["T3"], packed["w1"], packed["b1"]))
    out.update(h1=h1, h2=h2, c1=c1, c2=c2)
    out["T64"] = fc_head(wide_max(c2["y"], t64["w3"], t64["b3"], 1), t64).view(B, 64, 64)
    out["W3eff"] = torch.einsum("oj,bij->boi", packed["w3"], out["T64"])       # W3 (T64^T h2) = (W3 T64^T) h2
    (h3, h4), _ = chain([(out["W3eff"], packed["b3"]), (packed["w4"], packed["b4"])], X=h2["y"])
    out.update(h3=h3, h4=h4)
    out["logits"] = fc_head(wide_max(h4["y"], packed["w5"], packed["b5"], 3), packed)
    return out
