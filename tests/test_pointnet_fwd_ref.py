"""CPU: the float64 restatement of the PointNet forward's trunk (tests/_pointnet_fwd_ref.py) is the oracle's forward; the
bounds of tests/_pointnet_fwd_cases.py hold a plain fp32 evaluation, notice one defect of each kind, and leave at most 0.5 %
of a case's gate bits open.  What tests/test_gpu_pointnet_fwd.py holds the kernels to is exactly this."""
import pytest
import torch

from tests import _pointnet_fwd_cases as C
from tests import _pointnet_fwd_ref as R


def test_composed_restatement_is_the_oracle_forward():
    """The oracle exposes no intermediates: the restatement, stage after stage up to h4, then the float64 wide layer and head,
    gives the oracle's float64 logits (the folded weights are the project's fp32 ones: 2^-24 per weight)."""
    from oracle import geoa3_oracle as O
    from geoa3_amd.pointnet import pack_pointnet
    sd = O.make_pointnet_state_dict(40, seed=0)
    packed = pack_pointnet(sd)
    dbl = lambda p: {k: (dbl(v) if isinstance(v, dict) else v.double() if isinstance(v, torch.Tensor) and v.is_floating_point()
                         else v) for k, v in p.items()}
    for Bn, N in ((3, 77), (2, 300)):
        pc, _ = O.make_synthetic_clouds(Bn, N, seed=5 + N)
        want = O.pointnet_forward({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, pc.double())
        got = R.pointnet_trunk(dbl(packed), pc.double())
        assert got["h4"]["y"].shape == (Bn, 128, N) and got["T3"].shape == (Bn, 3, 3)
        err = float((got["logits"] - want).abs().max())
        print("restatement vs oracle (B %d, N %d): max |dlogits| = %.3g of %.3g" % (Bn, N, err, float(want.abs().max())))
        assert err <= 1e-5 * float(want.abs().max())


def test_gate_bit_packing_round_trip():
    gen = torch.Generator().manual_seed(3)
    for N in (1, 64, 77, 130):
        g = torch.rand(2, 5, N, generator=gen) < 0.5
        for tail in (True, False):
            assert torch.equal(R.unpack_gate_bits(R.pack_gate_bits(g, tail_ones=tail), N), g)


@pytest.mark.parametrize("kind", C.KINDS)
def test_open_gate_share_is_capped_for_every_case(kind):
    """|pre| within the bound of zero leaves a gate bit open: at most 0.5 % of a stage's bits in every case"""
    worst = 0.0
    for N in C.CHAIN_N:
        for v in C.variants(kind):
            _, (layers, _) = C.case_and_reference(kind, N, v)
            for i, L in enumerate(layers):
                share = float(R.undecided(L).double().mean())
                worst = max(worst, share)
                assert share <= C.OPEN_CAP, (kind, N, v, i, share)
    for big in (C.large_chain_case, C.large_conv_case):
        for L in big()[1][0]:
            share = float(R.undecided(L).double().mean())
            worst = max(worst, share)
            assert share <= C.OPEN_CAP, (big.__name__, share)
    print("largest open share %s: %.2e" % (kind, worst))


@pytest.mark.parametrize("kind", C.KINDS)
def test_plain_fp32_evaluation_stays_inside_every_bound(kind):
    """torch's fp32 evaluation of the same chain: every stage's values inside the bound, every decided gate the float64 one"""
    worst = 0.0
    for N in C.CHAIN_N:
        for v in C.variants(kind):
            c, (layers, _) = C.case_and_reference(kind, N, v)
            f32, _ = C.reference_of(c, dtype=torch.float32)
            for i, (L, F) in enumerate(zip(layers, f32)):
                ratio = R.worst_ratio(F["y"], L["y"], L["bound"])
                worst = max(worst, ratio)
                assert ratio <= 1.0, (kind, N, v, i, ratio)
                assert R.gate_ratio(F["pre"] > 0, L)[0] == 0, (kind, N, v, i)
    print("fp32 CPU evaluation, worst err/bound %s: %.4f" % (kind, worst))


def _noticed(c, layers, defect, stored_only=True):
    """does some stage's bound (values of the stored stages, decided gate bits of all) tell the defective chain apart?"""
    bad, _ = C.reference_of(c, defect=defect)
    stored = C.STORED[c["kind"]]
    for i, (L, D) in enumerate(zip(layers, bad)):
        if (stored[i] or not stored_only) and R.worst_ratio(D["y"], L["y"], L["bound"]) > 1.0:
            return True
        if R.gate_ratio(D["gate"], L)[0] > 0:
            return True
    return False


@pytest.mark.parametrize("kind", C.KINDS)
def test_each_bound_notices_one_defect_of_each_kind(kind):
    """a lost term (the largest input row of a stage, one coordinate of the first layer), T3 applied transposed, another
    stage's bias, instance 0's weights for every instance, the gate taken before the bias is added"""
    for N in C.CHAIN_N:
        for v in C.variants(kind):
            c, (layers, first) = C.case_and_reference(kind, N, v)
            tag = (kind, N, v)
            ns = len(layers)
            for i in range(ns):
                h = (first["y"] if first is not None else c["X"].double()) if i == 0 else layers[i - 1]["y"]
                k = int(h.abs().amax(dim=(0, 2)).argmax())
                assert _noticed(c, layers, (i, {"drop_term": k})), tag + ("lost term", i)
                assert _noticed(c, layers, (i, {"gate_before_bias": True})), tag + ("gate before bias", i)
                other = c["stages"][(i + 1) % ns][1] if ns > 1 else c["b1"]
                wrong = torch.zeros_like(c["stages"][i][1]).double()
                m = min(len(wrong), len(other))
                wrong[:m] = other[:m].double()
                assert _noticed(c, layers, (i, {"wrong_bias": wrong})), tag + ("wrong bias", i)
            if first is not None:
                assert _noticed(c, layers, ("first", {"drop_term": 0})), tag + ("lost coordinate",)
                if c["T3"] is not None:
                    assert _noticed(c, layers, ("first", {"T3_transposed": True})), tag + ("T3 transposed",)
            else:
                assert _noticed(c, layers, (0, {"instance0_weights": True})), tag + ("instance 0's weights",)
