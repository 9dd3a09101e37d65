"""CPU: the float64 statement of the first-layer data gradient (explain.conv_image_dgrad_np) against torch autograd through F.conv2d, the
refusals that come before any launch, and the consistency of the recorded tables of tests/explain_cnn_util.py."""
import numpy as np
import pytest
import torch

import explain_cnn_util as cu


@pytest.mark.parametrize("cin,cout,k,stride,pad,Hi", cu.DGRAD_CASES)
def test_conv_image_dgrad_np_is_autograd_through_conv2d(cin, cout, k, stride, pad, Hi):
    """to 1e-12 relative (of the largest entry), without and with std and scale_inv; the pixels no tap reaches are exactly 0"""
    from eoe_amd.explain import conv_image_dgrad_np
    n = 3
    dy, w = cu.dgrad_case(cin, cout, k, stride, pad, Hi, n)
    for std, scale_inv in ((None, 1.0), (cu.DGRAD_STD[:cin], 1.0 / 256.0), (cu.DGRAD_STD[:cin], 0.3)):
        got = conv_image_dgrad_np(dy, w, n, Hi, Hi, stride, pad, std, scale_inv)
        ref = cu.dgrad_autograd(dy, w, n, Hi, stride, pad, std, scale_inv)
        assert got.shape == ref.shape == (n, cin, Hi, Hi) and got.dtype == np.float64
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"[{cin}->{cout} k{k} s{stride} p{pad} {Hi}] std={std} scale_inv={scale_inv:g}: {err:.2e}")
        assert err <= 1e-12
    if (k, stride, pad, Hi) == (3, 2, 0, 6):
        assert (got[:, :, -1, :] == 0).all() and (got[:, :, :, -1] == 0).all() and np.abs(got[:, :, :-1, :-1]).min() > 0


def test_the_bound_covers_an_fp32_evaluation_of_the_statement():
    """the derived bound of the kernel test holds for the same sum taken in fp32 in another order (numpy einsum per tap)"""
    from eoe_amd.explain import conv_image_dgrad_np
    cin, cout, k, stride, pad, Hi = cu.DGRAD_CASES[0]
    dy, w = cu.dgrad_case(cin, cout, k, stride, pad, Hi, 1)
    ref = conv_image_dgrad_np(dy, w, 1, Hi, Hi, stride, pad)
    Ho = cu.out_size(Hi, k, stride, pad)
    full = np.zeros((1, cin, Hi + 2 * pad, Hi + 2 * pad), dtype=np.float32)
    for ky in range(k):
        for kx in range(k):
            full[:, :, ky:ky + Ho, kx:kx + Ho] += np.einsum("nhwo,oc->nchw", dy.reshape(1, Ho, Ho, cout), w[:, :, ky, kx])
    got = full[:, :, pad:pad + Hi, pad:pad + Hi]
    assert (np.abs(got - ref) <= cu.dgrad_bound(dy, w, 1, Hi, stride, pad, None, 1.0)).all()


def test_refusals_come_before_any_launch():
    """models on the CPU: a refusal that came behind a launch would fail as 'no GPU' instead"""
    from eoe_amd import explain
    from eoe_amd.models import CNN32, WideResNet
    wrn = WideResNet().train()
    with pytest.raises(NotImplementedError, match="residual junctions and CBAM") as e:
        explain.input_gradient(wrn, torch.zeros(1, 3, 224, 224), explain.score_fn("hsc"))
    assert "eval-mode" in str(e.value) and "pool" not in str(e.value) and wrn.training
    with pytest.raises(NotImplementedError, match="residual junctions and CBAM"):
        explain.input_gradient(torch.nn.Sequential(wrn), torch.zeros(1, 3, 224, 224), explain.score_fn("hsc"))
    with pytest.raises(NotImplementedError, match="VisualTransformer"):
        explain.attention_rollout(CNN32(), torch.zeros(1, 3, 32, 32))
    # a CNN32 passes the check; its forward then refuses the CPU tensor, with every flag back in place
    cnn = CNN32(bias=True).train()
    cnn.bn2d2.eval()
    with pytest.raises(RuntimeError, match="GPU only"):
        explain.input_gradient(cnn, torch.zeros(1, 3, 32, 32), explain.score_fn("hsc"))
    assert cnn.training and not cnn.bn2d2.training and all(p.requires_grad for p in cnn.parameters())


def test_the_trainer_accepts_the_cnns_for_explain_and_not_for_attention():
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN28, CNN32, WideResNet
    from eoe_amd.training import TRAINER

    class Src(ListSource):
        def test_inputs(self, rows):
            raise AssertionError("not reached")
    b = [(torch.zeros(2, 3, 32, 32), torch.tensor([0, 1]))]
    tr = TRAINER["hsc"](CNN32(), dataset=Src(b, b), classes=["only"], device="cpu", extremes=2, explain=True, attention=True)
    for m in (CNN32(), CNN28(bias=True)):
        tr._check_explainable(m, tr.ds)
        with pytest.raises(NotImplementedError, match="attention=True needs a ViT encoder"):
            tr._check_explainable(m, tr.ds, "attention", "whose attention could be rolled out")
    with pytest.raises(NotImplementedError, match="residual junctions and CBAM"):
        tr._check_explainable(WideResNet(), tr.ds)
    with pytest.raises(NotImplementedError, match="explain=True needs a ViT encoder or a CNN32 / CNN28"):
        tr._check_explainable(torch.nn.Linear(2, 2), tr.ds)


def test_the_recorded_floors_are_what_the_oracle_gives():
    """explain_cnn_util.FLOOR against a recomputation (the fp64 oracle against itself with 16-bit weights and convolution inputs)"""
    for dt, table in cu.FLOOR.items():
        assert set(table) == set(cu.CASES)
        for case, want in table.items():
            got = cu.floor(*case, dt)
            assert abs(got - want) <= 2e-3 * want, (dt, case, got, want)


def test_the_bars_follow_from_the_measured_tables():
    """fast mode: per (dtype, model) the bar is twice the worst measured value, and no measurement lies beyond 3 x its case's own floor;
    parity mode: twice the worst measured value, below the project's parity bar"""
    for dt, table in cu.INPUT_GRAD_MEASURED.items():
        assert set(table) == set(cu.CASES)
        for case, v in table.items():
            assert v <= cu.CEILING_FACTOR * cu.FLOOR[dt][case], (dt, case, v)
        for name in cu.MODELS:
            worst = max(v for (n, _, _), v in table.items() if n == name)
            assert cu.INPUT_GRAD_BAR[dt][name] == pytest.approx(2 * worst, rel=1e-6)
    for name in cu.MODELS:
        assert cu.PARITY_MEASURED[name] <= cu.PARITY_CEILING
        assert cu.PARITY_BAR[name] == pytest.approx(2 * cu.PARITY_MEASURED[name], rel=1e-6)


def test_the_saturated_cases_keep_the_score_derivative_inside_fp32():
    """explain_cnn_util.SATURATED_CASES by its own rule, on the fp64 oracle: |out| < 69 in every case (exp(-|out|) >= 2^-100, what the
    per-image seed brings to order one) with a score of 1 to fp32 rounding, and with fc2 x 64 a quarter of the chosen variance gain
    would leave |out| above 69"""
    def out_norms(name, gain, var_gain):
        m = cu.build(cu.omodels, name, True, gain, var_gain).double().eval()
        x = cu.images_of(name).double()
        mean, std = cu.normalize_of(name, True)
        c = x.shape[1]
        with torch.no_grad():
            return m((x - torch.tensor(mean).double().view(1, c, 1, 1)) / torch.tensor(std).double().view(1, c, 1, 1)).norm(dim=1)
    for name, gain, var_gain in cu.SATURATED_CASES:
        norms = out_norms(name, gain, var_gain)
        print(name, gain, var_gain, norms.tolist())
        assert 25.0 < float(norms.min()) and float(norms.max()) < 69.0
        if gain == 64.0:
            assert float(out_norms(name, gain, var_gain / 4).max()) > 69.0
            assert float(out_norms(name, gain, 1.0).min()) > 500.0
