"""CPU tier: the multi-scale-mode (MSM) API -- parsing, trainer construction, routing, the library's host operators against
numpy's fft-mask-ifft form and the g17 fixture, the blur k-rule and argument validation of the new entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import fill


def test_msm_parse_and_str_round_trip():
    from eoe_amd.msm import MSM
    for s in ("lpf+train_nominal--M4", "hpf+train_oe--M0", "blur+test_nominal--M8", "sharpen+test_anomalous--M2"):
        m = MSM.load(s)
        assert str(m) == s and repr(m) == s
    m = MSM.load("lpf+test_anomalous")
    assert m.magnitude is None and str(m) == "lpf+test_anomalous--MNone"
    assert MSM.load("hpf+train_oe--M16", load_magnitude=False).magnitude is None
    assert str(MSM("hpf", "train_oe").set_magnitude(3)) == "hpf+train_oe--M3"
    assert MSM("blur", "test_nominal", 2).ds_part == 2
    with pytest.raises(ValueError):
        MSM("median", "train_nominal")
    with pytest.raises(ValueError):
        MSM("lpf", "validation")
    with pytest.raises(ValueError):
        MSM.load("lpf+train_normal--M2")


def test_trainer_accepts_fft_and_blur_msms_and_refuses_sharpen():
    from eoe_amd.msm import MSM
    from eoe_amd.training import HSCTrainer
    model = torch.nn.Linear(2, 2)
    tr = HSCTrainer(model, dataset=None, msms=[MSM.load("lpf+train_nominal--M4")], device="cpu")
    assert [str(m) for m in tr.msms] == ["lpf+train_nominal--M4"]
    HSCTrainer(model, msms=[MSM.load("hpf+train_oe--M2"), MSM.load("blur+test_nominal--M1")], device="cpu")
    with pytest.raises(NotImplementedError, match="sharpen"):
        HSCTrainer(model, msms=[MSM.load("sharpen+train_nominal--M4")], device="cpu")


def test_routing_table_follows_the_reference():
    from eoe_amd.msm import MSM, routing
    msms = [MSM("lpf", "train_nominal", 4), MSM("hpf", "test_anomalous", 2), MSM("blur", "train_oe", 1),
            MSM("hpf", "train_nominal", 8), MSM("blur", "test_nominal", 3)]
    # train: nominal rows get train_nominal ops, OE rows get train_oe ops, in list order
    assert routing(msms, "train") == [("lpf", 4, True, False), ("blur", 1, False, True), ("hpf", 8, True, False)]
    assert routing(msms, "test") == [("hpf", 2, False, True), ("blur", 3, True, False)]
    assert routing([], "train") == []
    with pytest.raises(ValueError):
        routing(msms, "val")


def test_apply_msms_selects_rows_in_order(monkeypatch):
    """which rows of a [normal | OE] batch and of a test batch get which op, in which order"""
    from eoe_amd import msm
    calls = []

    def fake(x, op, mag, rows=None):
        calls.append((op, mag, None if rows is None else rows.tolist()))
        return x + 1

    monkeypatch.setattr(msm, "msm_filter", fake)
    imgs = torch.zeros((4, 1, 2, 2))
    lbls = torch.tensor([0, 0, 1, 1])
    msms = [msm.MSM("lpf", "train_nominal", 4), msm.MSM("blur", "train_oe", 1), msm.MSM("hpf", "test_nominal", 2),
            msm.MSM("hpf", "test_anomalous", 5)]
    out = msm.apply_msms(imgs, lbls, msms, "train", 0)
    assert calls == [("lpf", 4, [True, True, False, False]), ("blur", 1, [False, False, True, True])]
    assert float(out[0, 0, 0, 0]) == 2.0
    calls.clear()
    msm.apply_msms(imgs, torch.tensor([1, 0, 1, 0]), msms, "test", 0)
    assert calls == [("hpf", 2, [False, True, False, True]), ("hpf", 5, [True, False, True, False])]
    calls.clear()
    assert msm.apply_msms(imgs, lbls, msms[:1], "test", 0) is imgs and calls == []


def _dense_np(op, n, mag):
    """numpy's fft-mask-ifft form of the 1-D operator: F^-1 S^-1 diag(mask) S F"""
    e = min(mag, n // 2)
    i = np.arange(n)
    mask = ((i >= e) & (i < n - e)) if op == "lpf" else ((i >= n // 2 - e) & (i < n // 2 + e))
    eye = np.eye(n)
    return np.fft.ifft(np.fft.ifftshift(mask[:, None] * np.fft.fftshift(np.fft.fft(eye, axis=0), axes=0), axes=0), axis=0)


@pytest.mark.parametrize("n", [28, 31, 32, 224])
def test_host_operators_equal_numpy_fft_form(n):
    from eoe_amd.msm import host_operator
    for e in (1, 2, 4, 8, 16, 32, 64, 112, 256):
        for op in ("lpf", "hpf"):
            want = _dense_np(op, n, e)
            g, cs = host_operator(op, n, e, False)
            assert cs == (0.0, 1.0) and np.abs(g - want).max() < 1e-12, (op, n, e)
            u, (c, s) = host_operator(op, n, e, True)
            assert u.shape[1] <= n // 2 and (c, s) in ((0.0, 1.0), (1.0, -1.0))
            assert np.abs(c * np.eye(n) + s * (u @ u.conj().T) - want).max() < 1e-12, (op, n, e)


def test_numpy_form_matches_golden_fp64(golden):
    from eoe_amd.msm import fft_filter_np
    g = golden("g17_msm")
    for key in sorted(k for k in g if k.startswith("out64/")):
        _, op, size, mag = key.split("/")
        if size == "224":           # regenerated from its fill name; outputs kept on the [::8, ::8] grid (make_golden_msm.py)
            x = fill.fill("g17/224", (1, 1, 224, 224), std=0.25, mean=0.5).astype(np.float64)
        else:
            x = g[f"in64/{size}"]
            assert np.array_equal(x, fill.fill(f"g17/{size}", x.shape, std=0.25, mean=0.5).astype(np.float64))
        want = g[key]
        got = fft_filter_np(x, op, int(mag))
        if size == "224":
            got = got[:, :, ::8, ::8]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), key
        assert np.abs(got[~nan] - want[~nan]).max(initial=0.0) < 1e-12, key
    # ConditionalCompose(gpu=True): the filter on the rows whose label matches, the other on the rest
    x, y, want = g["compose/x"], g["compose/y"], g["compose/out"]
    a = fft_filter_np(x, "lpf", 4)
    b = fft_filter_np(x, "hpf", 2)
    sel = (y == 0)[:, None, None, None]
    got = np.where(sel, a, x)
    got = np.where(sel, got, fft_filter_np(got, "hpf", 2))
    assert np.abs(got - want).max() < 1e-12
    assert b.shape == x.shape


def test_blur_k_rule_matches_reference_formula():
    from eoe_amd.msm import blur_taps_k
    for sigma in (0.5, 1, 2, 3, 4, 7, 8, 16, 32, 64, 100, 128, 256):
        for w in (28, 32, 224):
            k_ref = 2 * int(int(sigma / 2) + 0.5) + 1
            k_ref = max(min(k_ref, 2 * int(int(w / 2) + 0.5) - 1), 3)
            assert blur_taps_k(sigma, w) == k_ref
    assert blur_taps_k(8, 32) == 9 and blur_taps_k(32, 32) == 31 and blur_taps_k(1, 32) == 3
    assert blur_taps_k(128, 224) == 129 and blur_taps_k(256, 224) == 223 and blur_taps_k(256, 28) == 27


def test_blur_workspace_takes_the_imagenet_magnitudes_at_224():
    """the ImageNet driver's blur magnitudes (multiscale_imagenet.py: up to 256) at 224^2: k = 65, 129 and 223 taps"""
    from eoe_amd import _lib
    lib = _lib.lib
    form, nb = C.c_int(-1), C.c_size_t(1)
    for sigma in (64, 128, 256):
        rc = lib.eoe_msm_workspace(3, 4, 3, 224, 224, sigma, C.byref(form), C.byref(nb))
        assert rc == 0, (sigma, lib.eoe_last_error())
        assert form.value == 0 and nb.value == 4 * 4 * 3 * 224 * 224, sigma


def test_blur_tap_limit_boundary():
    """the largest k the kernels take (223) is accepted, the next odd k (225: W = 226 at sigma 224) is refused, naming the
    limit"""
    from eoe_amd import _lib
    from eoe_amd.msm import blur_taps_k
    lib = _lib.lib
    form, nb = C.c_int(0), C.c_size_t(0)
    assert blur_taps_k(222, 226) == 223 and blur_taps_k(224, 226) == 225
    assert lib.eoe_msm_workspace(3, 2, 1, 226, 226, 222, C.byref(form), C.byref(nb)) == 0
    assert nb.value == 4 * 2 * 226 * 226
    assert lib.eoe_msm_workspace(3, 2, 1, 226, 226, 224, C.byref(form), C.byref(nb)) == 3
    assert b"225 taps (at most 223)" in lib.eoe_last_error()
    # the filter refuses it before touching the GPU
    assert lib.eoe_msm_filter(3, 16, 32, None, 2, 1, 226, 226, 224, None, 64, 1 << 30, None) == 3
    assert b"225 taps (at most 223)" in lib.eoe_last_error()


def test_msm_entry_points_validate_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    cols = C.c_int(0)
    assert lib.eoe_msm_operator(9, 32, 4, 0, None, None, C.byref(cols), None) == 1
    assert lib.eoe_msm_operator(1, 1, 4, 0, None, None, C.byref(cols), None) == 1
    assert lib.eoe_msm_operator(1, 32, 4, 2, None, None, C.byref(cols), None) == 1
    assert lib.eoe_msm_operator(1, 32, 4, 1, None, None, C.byref(cols), None) == 0 and cols.value == 8
    form, nb = C.c_int(0), C.c_size_t(0)
    assert lib.eoe_msm_workspace(1, 4, 3, 32, 32, 4, None, None) == 1
    assert lib.eoe_msm_workspace(7, 4, 3, 32, 32, 4, C.byref(form), C.byref(nb)) == 1
    assert lib.eoe_msm_workspace(1, 4, 3, 32, 16, 4, C.byref(form), C.byref(nb)) == 1 and b"square" in lib.eoe_last_error()
    assert lib.eoe_msm_workspace(1, 4, 3, 32, 32, 4, C.byref(form), C.byref(nb)) == 0 and form.value == 1 and nb.value == 0
    assert lib.eoe_msm_workspace(2, 4, 3, 224, 224, 8, C.byref(form), C.byref(nb)) == 0 and form.value == 2 and nb.value > 0
    assert lib.eoe_msm_workspace(3, 4, 3, 224, 224, 8, C.byref(form), C.byref(nb)) == 0 and nb.value == 4 * 4 * 3 * 224 * 224
    # the filter checks before touching the GPU: null / aliased buffers, missing workspace or operator
    assert lib.eoe_msm_filter(1, None, None, None, 4, 3, 32, 32, 4, None, None, 0, None) == 1
    assert lib.eoe_msm_filter(1, 16, 16, None, 4, 3, 32, 32, 4, None, None, 0, None) == 1
    assert lib.eoe_msm_filter(1, 16, 32, None, 4, 3, 32, 32, 4, None, None, 0, None) == 1 and b"operator" in lib.eoe_last_error()
    assert lib.eoe_msm_filter(2, 16, 32, None, 4, 3, 224, 224, 4, 64, None, 0, None) == 1 and b"workspace" in lib.eoe_last_error()
    assert lib.eoe_msm_filter(1, 16, 32, None, 0, 3, 32, 32, 4, 64, None, 0, None) == 1


def test_msm_filter_refuses_cpu_tensors():
    from eoe_amd.msm import msm_filter
    with pytest.raises(RuntimeError):
        msm_filter(torch.zeros((1, 3, 32, 32)), "lpf", 4)
    with pytest.raises(ValueError):
        msm_filter(torch.zeros((1, 3, 32, 32)), "sharpen", 4)
