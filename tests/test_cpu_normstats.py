"""CPU tier: per-task normalisation ('normalize' / 'gcn-normalize') -- the g20 fixture's self-consistency, mode strings, argument
validation of the two new entry points, and the host half of `fit_statistics` (the RunningStats recurrence and the GCN extremes
from exact integer sums, which has no kernel in it) against the reference's results."""
import ctypes as C

import numpy as np
import pytest
import torch

import normstats_util as nu


def test_fixture_is_self_consistent(golden):
    g = golden("g20_normstats")
    for case in nu.STATS_CASES:
        for k in ("mean", "std", "tmin", "tmax", "range"):
            a, b = np.asarray(g[f"stats/{case}/{k}32"], np.float64), np.asarray(g[f"stats/{case}/{k}64"], np.float64)
            noise = float(g[f"noise/stats/{case}/{k}"])
            assert 0.0 < noise < 1e-5 and np.max(np.abs(a - b) / np.abs(b)) <= noise * (1 + 1e-12), (case, k)
        assert g[f"stats/{case}/tmax64"] == g[f"stats/{case}/tmin64"] + g[f"stats/{case}/range64"]
    # the ramp makes RunningStats' batch-mean weighting visible: a textbook reduction cannot meet this case
    assert np.abs(g["stats/ramp37/mean64"] - g["stats/ramp37/plain_mean"]).max() > 1e-3
    plain = nu.stats_set("ramp37").astype(np.float64).mean(axis=(0, 1, 2)) / 255.0
    assert np.allclose(plain, g["stats/ramp37/plain_mean"], rtol=0, atol=1e-15)
    assert len(g["stats/ramp37_idx20/index"]) == 20 and (np.diff(g["stats/ramp37_idx20/index"]) > 0).all()
    for size, shape in nu.OP_SHAPES.items():
        for scale in ("l1", "l2"):
            for affine in (0, 1):
                y64 = g[f"op/{size}/{scale}/{affine}/y64"]
                want = (shape[0], shape[1], 28, 28) if size == "224" else shape
                assert y64.shape == want and y64.dtype == np.float64 and np.isfinite(y64).all()
                noise = float(g[f"noise/op/{size}/{scale}/{affine}"])
                assert 0.0 < noise < 1e-4
                if size != "32":                 # the fp32 outputs of the largest case are left out (file size), its noise is stored
                    y32 = g[f"op/{size}/{scale}/{affine}/y32"].astype(np.float64)
                    assert np.max(np.abs(y32 - y64) / np.maximum(1.0, np.abs(y64))) <= noise * (1 + 1e-12)
    assert g["traj/losses"].shape == (nu.TRAJ_STEPS,) and g["traj/scores64"].shape == (nu.TRAJ_STEPS, 2 * nu.TRAJ_HALF)
    assert np.abs(g["traj/losses"] - g["traj/losses64"]).max() > 0.0


def test_mode_strings():
    from eoe_amd.normalize import norm_mode, NORM_MODES, STD_NORM, GCN_NORM
    assert sorted(NORM_MODES) == ["gcn-norm", "gcn-normalise", "gcn-normalize", "norm", "normalise", "normalize"]
    for s in ("norm", "normalise", "normalize", "Normalize"):
        assert norm_mode(s) == STD_NORM == 0
    for s in ("gcn-norm", "gcn-normalise", "gcn-normalize", "GCN-Normalize"):
        assert norm_mode(s) == GCN_NORM == 1
    with pytest.raises(ValueError) as e:
        norm_mode("standardize")
    for s in NORM_MODES:
        assert s in str(e.value)
    with pytest.raises(ValueError):
        norm_mode(None)


def _u8(n=4, hw=8):
    return torch.zeros((n, hw, hw, 3), dtype=torch.uint8)


def test_source_refuses_normalize_with_mean_and_wrong_mode_statistics():
    """both are decided before anything touches the device"""
    from eoe_amd.data import ResidentImageSource, LabelledImageSet
    from eoe_amd.normalize import check_ds_statistics
    kw = dict(crop=8, device="cpu")
    lab = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="mean"):
        ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="normalize", mean=[0.5] * 3, std=[0.2] * 3, **kw)
    with pytest.raises(ValueError, match="mode"):
        ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="gcn-normalize",
                            ds_statistics={"mean": [0.5] * 3, "std": [0.2] * 3, "mode": 0}, **kw)
    with pytest.raises(ValueError, match="mode"):
        ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="normalize",
                            ds_statistics={"mean": [-1.0] * 3, "std": [4.0] * 3, "mode": 1}, **kw)
    with pytest.raises(ValueError, match="valid strings"):
        ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="zscore", **kw)
    with pytest.raises(ValueError):
        ResidentImageSource(_u8(), _u8(), _u8(), lab, ds_statistics={"mean": [0.5] * 3, "std": [0.2] * 3, "mode": 0}, **kw)
    # given statistics win over fitting (no kernel runs: this is a CPU-resident set) and come back as plain Python values
    st = {"mean": torch.tensor([-1.5, -1.5, -1.5]), "std": np.array([4.0, 4.0, 4.0]), "mode": 1}
    src = ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="gcn-norm", ds_statistics=st, **kw)
    assert src.ds_statistics == {"mean": [-1.5] * 3, "std": [4.0] * 3, "mode": 1}
    assert all(type(v) is float for v in src.ds_statistics["mean"] + src.ds_statistics["std"]) and type(src.ds_statistics["mode"]) is int
    assert src.mean is None and src.normalize.shift == [-1.5] * 3 and src.normalize.range == [4.0] * 3 and src.normalize.scale == "l1"
    src.defer_normalize(True)
    assert src.normalize.shift == [-1.5] * 3                       # the MSM path does not drop the operator
    src = ResidentImageSource(_u8(), _u8(), _u8(), lab, normalize="normalize", ds_statistics={"mean": [0.4] * 3, "std": [0.2] * 3}, **kw)
    assert src.mean == [0.4] * 3 and src.std == [0.2] * 3 and src.normalize is None and src.ds_statistics["mode"] == 0
    assert check_ds_statistics({"mean": [0.0], "std": [1.0]}, 0)["mode"] == 0
    # a set built with ready mean= / std= keeps them when a snapshot brings statistics along (every reference snapshot does)
    plain = LabelledImageSet(_u8(), lab, _u8(), lab, _u8(), ["a"], 8, device="cpu", mean=[0.3] * 3, std=[0.1] * 3)
    src = plain.source([0], 0, ds_statistics=st)
    assert src.mean == [0.3] * 3 and src.std == [0.1] * 3 and src.ds_statistics is None and src.normalize is None


def test_new_entry_points_validate_arguments():
    from eoe_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5            # additive: the ABI version does not move
    # eoe_set_moments_u8(src, n_src, H, W, C, index, n_index, chan_sums, img_stats, stream)
    assert lib.eoe_set_moments_u8(16, 4, 8, 8, 2, None, 4, 32, 48, None) == 1 and b"C must be 1 or 3" in lib.eoe_last_error()
    assert lib.eoe_set_moments_u8(None, 4, 8, 8, 3, None, 4, 32, 48, None) == 1 and b"null" in lib.eoe_last_error()
    assert lib.eoe_set_moments_u8(16, 4, 8, 8, 3, None, 4, None, 48, None) == 1 and b"null" in lib.eoe_last_error()
    assert lib.eoe_set_moments_u8(16, 4, 8, 8, 3, None, 4, 32, None, None) == 1
    assert lib.eoe_set_moments_u8(16, 0, 8, 8, 3, None, 4, 32, 48, None) == 1
    assert lib.eoe_set_moments_u8(16, 4, 0, 8, 3, None, 4, 32, 48, None) == 1
    assert lib.eoe_set_moments_u8(16, 4, 8, 8, 3, None, 0, 32, 48, None) == 1 and b"n_index" in lib.eoe_last_error()
    assert lib.eoe_set_moments_u8(16, 4, 1 << 14, 1 << 14, 3, None, 4, 32, 48, None) == 1 and b"at most" in lib.eoe_last_error()
    # eoe_gcn_normalize(x, y, n, C, H, W, scale, shift, range, stream)
    assert lib.eoe_gcn_normalize(16, 32, 4, 2, 8, 8, 1, None, None, None) == 1 and b"C must be 1 or 3" in lib.eoe_last_error()
    assert lib.eoe_gcn_normalize(None, 32, 4, 3, 8, 8, 1, None, None, None) == 1 and b"null" in lib.eoe_last_error()
    assert lib.eoe_gcn_normalize(16, None, 4, 3, 8, 8, 1, None, None, None) == 1
    assert lib.eoe_gcn_normalize(16, 32, 4, 3, 8, 8, 0, None, None, None) == 1 and b"unknown scale" in lib.eoe_last_error()
    assert lib.eoe_gcn_normalize(16, 32, 4, 3, 8, 8, 3, None, None, None) == 1 and b"unknown scale" in lib.eoe_last_error()
    assert lib.eoe_gcn_normalize(16, 32, 4, 3, 8, 8, 1, 64, None, None) == 1 and b"both or neither" in lib.eoe_last_error()
    assert lib.eoe_gcn_normalize(16, 32, 0, 3, 8, 8, 1, None, None, None) == 1
    assert lib.eoe_gcn_normalize(16, 32, 4, 3, 8, 0, 2, None, None, None) == 1
    assert {"eoe_set_moments_u8", "eoe_gcn_normalize"} <= set(_lib.header_symbols())


def _integer_sums(u8):
    """what eoe_set_moments_u8 returns, by numpy"""
    v = u8.astype(np.int64)
    m, H, W, Cc = v.shape
    chan = np.stack([v.sum(axis=(1, 2)), (v * v).sum(axis=(1, 2))], axis=2)               # [m, C, 2]
    S = v.reshape(m, -1).sum(1)
    N = H * W * Cc
    dev = np.abs(N * v.reshape(m, -1) - S[:, None]).sum(1)
    img = np.stack([v.reshape(m, -1).min(1), v.reshape(m, -1).max(1), dev], axis=1)
    return chan, img, S, N


@pytest.mark.parametrize("case", nu.STATS_CASES)
def test_host_recurrence_reproduces_the_reference(golden, case):
    """the host half of fit_statistics fed with numpy's integer sums: within max(3 x the reference's own fp32 noise, one fp32 ulp)
    of the fp64 twin, both modes"""
    from eoe_amd.normalize import running_stats_from_sums, gcn_extremes_from_stats
    g = golden("g20_normstats")
    name, idx = nu.stats_index(case)
    u8 = nu.stats_set(name)
    if idx is not None:
        assert np.array_equal(idx, g[f"stats/{case}/index"])
        u8 = u8[idx]
    chan, img, S, N = _integer_sums(u8)
    mean, std = running_stats_from_sums(chan, u8.shape[1] * u8.shape[2])
    print("\n   " + nu.check_stats_dict({"mean": list(mean), "std": list(std), "mode": 0}, g, case, 0, "host "))
    tmin, tmax = gcn_extremes_from_stats(img, S, N)
    c = u8.shape[3]
    print("   " + nu.check_stats_dict({"mean": [tmin] * c, "std": [tmax - tmin] * c, "mode": 1}, g, case, 1, "host "))
    # and the recurrence restated on images (tests' yardstick for sources) agrees with the twin as well
    m2, s2 = nu.running_stats_np(u8.transpose(0, 3, 1, 2).astype(np.float32).__truediv__(np.float32(255)).astype(np.float64))
    assert np.abs(m2 - g[f"stats/{case}/mean64"]).max() < 1e-13 and np.abs(s2 - g[f"stats/{case}/std64"]).max() < 1e-13


def test_textbook_statistics_would_fail_the_ramp_case(golden):
    g = golden("g20_normstats")
    plain = nu.stats_set("ramp37").astype(np.float64).mean(axis=(0, 1, 2)) / 255.0
    assert nu.stats_ratio(plain, g, "ramp37", "mean") > 1000.0


def test_cpu_tensors_are_refused():
    from eoe_amd.normalize import gcn_normalize, fit_statistics, GlobalContrastNormalization, GcnNormalize
    x = torch.rand((2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="GPU"):
        gcn_normalize(x)
    with pytest.raises(RuntimeError, match="GPU"):
        GlobalContrastNormalization()(x)
    with pytest.raises(RuntimeError, match="GPU"):
        GcnNormalize([0.0] * 3, [1.0] * 3)(x)
    with pytest.raises(RuntimeError, match="GPU"):
        fit_statistics(_u8())
    with pytest.raises(ValueError):
        fit_statistics(_u8(), mode="whiten")
    assert GlobalContrastNormalization(scale="l2").scale == "l2"
    GlobalContrastNormalization(GlobalContrastNormalization(scale="l1"), scale="l1")           # the reference's constructor
    with pytest.raises(AssertionError):
        GlobalContrastNormalization(GlobalContrastNormalization(scale="l2"), scale="l1")


def test_torch_formulation_matches_the_fixture(golden):
    """the torch-op chain the GPU tests and the bench use as yardstick IS the reference's formulation: in fp64 on the CPU it
    reproduces the twins"""
    from normstats_util import torch_gcn_normalize
    g = golden("g20_normstats")
    sh, rg = float(g["op/shift"]), float(g["op/range"])
    for size in ("32", "28"):
        x = torch.from_numpy(nu.op_input(size)).double()
        c = x.shape[1]
        for scale in ("l1", "l2"):
            got = torch_gcn_normalize(x, scale).numpy()
            assert np.abs(got - g[f"op/{size}/{scale}/0/y64"]).max() < 1e-11
            got = torch_gcn_normalize(x, scale, [sh] * c, [rg] * c).numpy()
            assert np.abs(got - g[f"op/{size}/{scale}/1/y64"]).max() < 1e-11
