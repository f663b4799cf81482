"""Checkers of the fused EdgeConv kernels (csrc/edgeconv.hip) and of geoa3_amd.dgcnn.DGCNN, written from the kernels' contract
(include/geoa3_hip.h) and from the public DGCNN classification model (Wang et al. 2019):

    edge_max / edge_max_grad   float32 numpy loops, one rounding per operation, sums in ascending (point, slot) order
    edgeconv_f64               the STANDARD formulation of one eval-mode layer in float64 torch -- cat([x_j - x_i ; x_i]),
                               conv2d, batch_norm, leaky_relu, max over the neighbours -- with the neighbour table given, and
                               the quantities the rounding bound of tests/test_gpu_edgeconv.py needs
    dgcnn_f64                  the whole eval-mode forward in float64 from a module's state_dict, the four tables given
"""
import numpy as np
import torch
import torch.nn.functional as TF

F = np.float32
SLOPE = F(0.2)
EDGE_LAYERS = ((6, 64), (128, 64), (128, 128), (256, 256))


def lrelu32(a):
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        return np.where(a > 0, a, (a * SLOPE).astype(F)).astype(F)


def edge_max(U, V, t, idx):
    """U, V [B,N,C] float32, t [C], idx int [B,N,k] -> (y [B,C,N] float32, arg int32 [B,N,C])"""
    U, V, t = np.asarray(U, F), np.asarray(V, F), np.asarray(t, F)
    B, N, C = U.shape
    k = idx.shape[2]
    y, arg = np.empty((B, C, N), F), np.empty((B, N, C), np.int32)
    for b in range(B):
        for i in range(N):
            best, a, bad = None, np.zeros(C, np.int32), False
            for s in range(k):
                j = int(idx[b, i, s])
                if not 0 <= j < N:
                    a[:], bad = s, True
                    break
                u = U[b, j]
                if s == 0:
                    best = u.copy()
                    continue
                take = (u > best) | (np.isnan(u) & ~np.isnan(best))     # the FIRST maximum; a NaN, once met, stays
                best, a = np.where(take, u, best), np.where(take, s, a).astype(np.int32)
            arg[b, i] = a
            if bad:
                y[b, :, i] = np.nan
            else:
                with np.errstate(all="ignore"):
                    pre = (best + V[b, i]).astype(F)
                    pre = (pre + t).astype(F)
                y[b, :, i] = lrelu32(pre)
    return y, arg


def edge_max_grad(g, y, arg, idx):
    """g, y [B,C,N] float32, arg [B,N,C], idx [B,N,k] -> (dU, dV) [B,N,C] float32"""
    g, y = np.asarray(g, F), np.asarray(y, F)
    B, C, N = g.shape
    k = idx.shape[2]
    with np.errstate(all="ignore"):
        dV = np.where(y > 0, g, (g * SLOPE).astype(F)).astype(F).transpose(0, 2, 1).copy()
    dU = np.zeros((B, N, C), F)
    for b in range(B):
        for i in range(N):
            for s in range(k):
                j = int(idx[b, i, s])
                if not 0 <= j < N:
                    continue
                m = arg[b, i] == s
                with np.errstate(all="ignore"):
                    dU[b, j, m] = (dU[b, j, m] + dV[b, i, m]).astype(F)
    return dU, dV


def bn_affine(sd, name, eps=1e-5):
    """(scale, shift) float64 of an eval-mode BatchNorm of a state_dict"""
    s = sd[name + ".weight"].double() / torch.sqrt(sd[name + ".running_var"].double() + eps)
    return s, sd[name + ".bias"].double() - sd[name + ".running_mean"].double() * s


def edgeconv_f64(x, idx, w, bn_w, bn_b, bn_m, bn_v, eps=1e-5):
    """One eval-mode EdgeConv layer, the standard formulation, float64.  x [B,C,N], idx int64 [B,N,k] (all valid),
    w [C',2C] -> dict: y [B,C',N]; arg [B,N,C'] (first maximum); gap [B,N,C'], best minus second-best pre-activation over
    the DISTINCT neighbours (inf where there is one); A [B,N,k,C'], the sum of the absolute values of the terms of
    U[j] + V[i] + t for every edge."""
    x, w = x.double(), w.double()
    B, C, N = x.shape
    k = idx.shape[2]
    xt = x.transpose(1, 2)                                                        # [B,N,C]
    xj = torch.gather(xt, 1, idx.reshape(B, N * k, 1).expand(B, N * k, C)).view(B, N, k, C)
    xi = xt.unsqueeze(2).expand(B, N, k, C)
    e = torch.cat((xj - xi, xi), 3).permute(0, 3, 1, 2)                           # [B,2C,N,k]
    pre = TF.batch_norm(TF.conv2d(e, w.view(w.shape[0], 2 * C, 1, 1)), bn_m.double(), bn_v.double(), bn_w.double(),
                        bn_b.double(), False, 0.0, eps)
    act = TF.leaky_relu(pre, 0.2)                                                 # [B,C',N,k]
    y, arg = act.max(3)
    # first maximum (torch.max promises no particular index among equals)
    arg = (act == y.unsqueeze(3)).to(torch.int64).argmax(3)
    s = bn_w.double() / torch.sqrt(bn_v.double() + eps)
    t = bn_b.double() - bn_m.double() * s
    wa, wd = w[:, :C] * s.view(-1, 1), (w[:, C:] - w[:, :C]) * s.view(-1, 1)
    A = (torch.einsum("oc,bnkc->bnko", wa.abs(), xj.abs()) + torch.einsum("oc,bnc->bno", wd.abs(), xt.abs()).unsqueeze(2) +
         t.abs().view(1, 1, 1, -1))
    p = pre.permute(0, 2, 3, 1)                                                   # [B,N,k,C']
    jbest = torch.gather(idx.unsqueeze(3).expand(B, N, k, p.shape[3]), 2, arg.permute(0, 2, 1).unsqueeze(2))   # [B,N,1,C']
    other = idx.unsqueeze(3) != jbest                                             # slots that hold ANOTHER point
    top = torch.gather(p, 2, arg.permute(0, 2, 1).unsqueeze(2)).squeeze(2)
    second = torch.where(other, p, torch.full_like(p, -float("inf"))).max(2)[0]
    return {"y": y, "arg": arg.permute(0, 2, 1), "gap": top - second, "A": A}


def dgcnn_f64(sd, x, idxs, emb_dims=1024):
    """The public model's eval-mode forward in float64: sd a state_dict, x [B,3,N], idxs the four tables ->
    (logits [B,classes], [the four EdgeConv outputs])."""
    sd = {k: v.detach().cpu() for k, v in sd.items()}
    h = x.double()
    feats = []
    for l, (cin, cout) in enumerate(EDGE_LAYERS, 1):
        p = "conv%d.1." % l
        h = edgeconv_f64(h, idxs[l - 1], sd["conv%d.0.weight" % l].view(cout, cin), sd[p + "weight"], sd[p + "bias"],
                         sd[p + "running_mean"], sd[p + "running_var"])["y"]
        feats.append(h)
    z = TF.conv1d(torch.cat(feats, 1), sd["conv5.0.weight"].double())
    z = TF.leaky_relu(TF.batch_norm(z, sd["conv5.1.running_mean"].double(), sd["conv5.1.running_var"].double(),
                                    sd["conv5.1.weight"].double(), sd["conv5.1.bias"].double(), False, 0.0, 1e-5), 0.2)
    z = torch.cat((z.max(2)[0], z.mean(2)), 1)
    for lin, bn in (("linear1", "bn6"), ("linear2", "bn7")):
        b = sd.get(lin + ".bias")
        z = TF.linear(z, sd[lin + ".weight"].double(), None if b is None else b.double())
        z = TF.leaky_relu(TF.batch_norm(z, sd[bn + ".running_mean"].double(), sd[bn + ".running_var"].double(),
                                        sd[bn + ".weight"].double(), sd[bn + ".bias"].double(), False, 0.0, 1e-5), 0.2)
    return TF.linear(z, sd["linear3.weight"].double(), sd["linear3.bias"].double()), feats
