"""CPU: the attention-rollout entry points exist and refuse bad arguments before any launch, the numpy statements on hand-worked
examples, the bars of tests/rollout_util.py against a fresh measurement, and the refusals of eoe_amd.explain and the trainer."""
import numpy as np
import pytest
import torch

import rollout_util as ru

NEW_SYMBOLS = ("eoe_attn_probs", "eoe_rollout_step", "eoe_rollout_map")
P, Q, R = 0x1000, 0x200000, 0x400000          # non-null, 16-byte aligned addresses nothing reads: every call below fails its checks first


def test_the_three_entry_points_are_exported_and_the_abi_version_stays():
    import eoe_amd
    from eoe_amd import _lib, explain
    assert _lib.lib.eoe_abi_version() == 5 and _lib.ABI_VERSION == 5
    declared = _lib.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and name in declared and hasattr(_lib.lib, name)
    assert (_lib.EOE_FUSE_MEAN, _lib.EOE_FUSE_MAX, _lib.EOE_FUSE_MIN) == (0, 1, 2)
    assert explain.FUSE == {"mean": 0, "max": 1, "min": 2}
    assert eoe_amd.attention_rollout is explain.attention_rollout and "attention_rollout" in eoe_amd.__all__


def test_attn_probs_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_attn_probs, lib.eoe_last_error
    # (qkv, probs, n, L, heads, dtype, fuse, stream)
    assert f(None, Q, 1, 50, 12, 1, 0, None) == 1 and b"null" in err()
    assert f(P, None, 1, 50, 12, 1, 0, None) == 1 and b"null" in err()
    for n in (0, -1):
        assert f(P, Q, n, 50, 12, 1, 0, None) == 1 and b"n must be positive" in err()
    for L in (0, -3, 641):
        assert f(P, Q, 1, L, 12, 1, 0, None) == 1 and b"sequence length" in err()
    for heads in (0, -1):
        assert f(P, Q, 1, 50, heads, 1, 0, None) == 1 and b"heads" in err()
    for dtype in (0, 3, 7):
        assert f(P, Q, 1, 50, 12, dtype, 0, None) == 1 and b"dtype" in err()
    for fuse in (-1, 3):
        assert f(P, Q, 1, 50, 12, 1, fuse, None) == 1 and b"fuse" in err()


def test_rollout_step_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_rollout_step, lib.eoe_last_error
    # (probs, r_in, r_out, n, L, residual, stream)
    assert f(None, Q, R, 1, 50, 0.5, None) == 1 and b"null" in err()
    assert f(P, Q, None, 1, 50, 0.5, None) == 1 and b"null" in err()
    assert f(P, Q, R, 0, 50, 0.5, None) == 1 and b"n must be" in err()
    for L in (0, 641):
        assert f(P, Q, R, 1, L, 0.5, None) == 1 and b"sequence length" in err()
    for residual in (1.0, -0.1, 1.5, float("nan")):
        assert f(P, Q, R, 1, 50, residual, None) == 1 and b"residual must be in [0, 1)" in err()
    assert f(P, R, R, 1, 50, 0.5, None) == 1 and b"must not alias r_in" in err()
    assert f(P, R + 16, R, 1, 50, 0.5, None) == 1 and b"must not alias r_in" in err()          # overlapping, not only equal
    assert f(R, Q, R, 1, 50, 0.5, None) == 1 and b"must not alias probs" in err()


def test_rollout_map_refuses_bad_arguments_before_any_launch():
    from eoe_amd._lib import lib
    f, err = lib.eoe_rollout_map, lib.eoe_last_error
    # (r, maps, n, L, grid, patch, stream)
    assert f(None, Q, 1, 50, 7, 32, None) == 1 and b"null" in err()
    assert f(P, None, 1, 50, 7, 32, None) == 1 and b"null" in err()
    assert f(P, Q, 0, 50, 7, 32, None) == 1 and b"n must be positive" in err()
    for L, grid in ((49, 7), (51, 7), (50, 8), (1, 0), (50, -7), (641, 25), (0, 0)):
        assert f(P, Q, 1, L, grid, 32, None) == 1 and (b"grid^2 + 1" in err() or b"sequence length" in err()), (L, grid)
    for patch in (0, -4, 1025):
        assert f(P, Q, 1, 50, 7, patch, None) == 1 and b"patch" in err()
    assert f(P, Q, 1 << 16, 626, 25, 1024, None) == 1 and b"32-bit indexing" in err()


# ------------------------------------------------------------------------------------------------ the numpy statements
def test_attention_probs_np_on_hand_worked_examples():
    from eoe_amd.explain import attention_probs_np
    # L = 2, one head: q rows (0, ...) and (8, 0, ...), k rows (1, 0, ...) and (0, ...): logits q k^T / 8 = [[0, 0], [1, 0]]
    qkv = np.zeros((2, 192))
    qkv[1, 0] = 8.0
    qkv[0, 64] = 1.0
    e = np.e
    want = np.array([[[0.5, 0.5], [e / (1 + e), 1 / (1 + e)]]])
    for fuse in ru.FUSES:
        np.testing.assert_allclose(attention_probs_np(qkv, 1, 2, 1, fuse), want, rtol=1e-15)
    assert np.array_equal(attention_probs_np(np.random.default_rng(0).normal(size=(1, 192)), 1, 1, 1), np.ones((1, 1, 1)))
    # two heads: head 0 as above, head 1 all-zero logits (uniform)
    two = np.zeros((2, 384))
    two[1, 0], two[0, 128] = 8.0, 1.0
    half = np.full((2, 2), 0.5)
    np.testing.assert_allclose(attention_probs_np(two, 1, 2, 2, "mean")[0], (want[0] + half) / 2, rtol=1e-15)
    np.testing.assert_allclose(attention_probs_np(two, 1, 2, 2, "max")[0], np.maximum(want[0], half), rtol=1e-15)
    np.testing.assert_allclose(attention_probs_np(two, 1, 2, 2, "min")[0], np.minimum(want[0], half), rtol=1e-15)
    with pytest.raises(ValueError, match="fuse"):
        attention_probs_np(qkv, 1, 2, 1, "median")


def test_attention_rollout_np_on_hand_worked_examples():
    from eoe_amd.explain import attention_rollout_np, rollout_matrix_np
    eye = np.eye(5)[None]
    assert np.array_equal(attention_rollout_np([eye, eye], 0.0, 2, 3), np.zeros((1, 6, 6)))          # R = I: the class row sees no patch
    r1 = rollout_matrix_np(eye, 0.0)
    assert np.array_equal(r1, eye)
    # a zero row and a NaN row are identity rows; the others are divided by their sums
    p = np.array([[[0.0, 0.0], [1.0, 3.0]]])
    np.testing.assert_allclose(rollout_matrix_np(p, 0.0)[0], [[1, 0], [0.25, 0.75]], rtol=1e-15)
    np.testing.assert_allclose(rollout_matrix_np(p, 0.5)[0], [[1, 0], [0.5 / 2.5, 2.0 / 2.5]], rtol=1e-15)
    assert np.array_equal(rollout_matrix_np(np.array([[[np.nan, 1.0], [0.5, 0.5]]]), 0.0)[0], [[1, 0], [0.5, 0.5]])
    # two layers, L = 2 (grid 1), residual 0.5: A^_1 = [[.75, .25], [.25, .75]], A^_2 = [[.5, .5], [0, 1]];  R = A^_2 A^_1
    p1 = np.array([[[0.5, 0.5], [0.5, 0.5]]])
    p2 = np.array([[[0.0, 1.0], [0.0, 1.0]]])
    m = attention_rollout_np([p1, p2], 0.5, 1, 2)
    np.testing.assert_allclose(m, np.full((1, 2, 2), 0.5 * 0.25 + 0.5 * 0.75), rtol=1e-15)
    # the map: class row, class column dropped, blocks constant
    r = np.arange(25, dtype=np.float64).reshape(1, 5, 5) + 1
    got = attention_rollout_np([r], 0.0, 2, 2)
    row = r[0, 0] / r[0, 0].sum()
    assert got.shape == (1, 4, 4)
    np.testing.assert_allclose(got[0], np.repeat(np.repeat(row[1:].reshape(2, 2), 2, 0), 2, 1), rtol=1e-15)
    with pytest.raises(ValueError, match="grid"):
        attention_rollout_np([r], 0.0, 3, 2)
    with pytest.raises(ValueError, match="residual"):
        attention_rollout_np([r], 1.0, 2, 2)


def test_the_bars_follow_from_a_fresh_measurement():
    """the measurement behind PROBS_BAR and STEP_BAR again, on the cases that set them and a few around: the constants are 4 x the
    measured error (BLAS builds order fp32 sums differently: within a factor of two)"""
    from eoe_amd.explain import attention_probs_np
    assert ru.PROBS_BAR == pytest.approx(4 * ru.PROBS_MEASURED) and ru.STEP_BAR == pytest.approx(4 * ru.STEP_MEASURED)
    worst = 0.0
    for L, heads, n in ((2, 1, 1), (63, 3, 3), (197, 12, 1), (640, 12, 1)):
        for dt in ru.DTYPES:
            for kind in ru.KINDS:
                q = ru.qkv_case(L, heads, n, dt, kind).float().numpy()
                for fuse in ru.FUSES:
                    worst = max(worst, np.abs(ru.probs_np32(q, n, L, heads, fuse) - attention_probs_np(q, n, L, heads, fuse)).max())
    assert ru.PROBS_MEASURED / 2 <= worst <= ru.PROBS_MEASURED * 2, worst
    worst = 0.0
    for L, n in ((2, 1), (50, 3), (640, 1)):
        for res in ru.RESIDUALS:
            for kind in ru.STEP_KINDS:
                ch = ru.step_chain_case(L, n, kind)
                a, b = ru.rollout_chain_np(ch, res, np.float64), ru.rollout_chain_np(ch, res, np.float32)
                worst = max(worst, max(np.abs(a[s] - b[s]).max() for s in (0, 3)))
    assert ru.STEP_MEASURED / 2 <= worst <= ru.STEP_MEASURED * 2, worst


def test_the_float64_tower_restatement_agrees_with_the_oracle_attention():
    """rollout_util's own restatement of the tower: with start_layer = -1 and residual 0 the map is the last block's class-token attention,
    renormalised over the patches' share"""
    from eoe_amd.models import ClipViTB32Custom
    kw, res, patch, heads = ru.TOWERS["narrow65"]
    torch.manual_seed(1)
    m = ClipViTB32Custom(**kw)
    maps, probs = ru.tower_rollout_f64(m.state_dict(), ru.tower_images("narrow65", 2), patch, heads, 2, residual=0.0, start_layer=-1)
    assert len(probs) == 1 and probs[0].shape == (2, 65, 65) and maps.shape == (2, 32, 32)
    np.testing.assert_allclose(probs[0].sum(axis=2), 1.0, rtol=1e-12)
    np.testing.assert_allclose(maps[:, ::4, ::4].reshape(2, 64), probs[0][:, 0, 1:], rtol=1e-12)


# ------------------------------------------------------------------------------------------------ refusals
def test_attention_rollout_refuses_a_cnn_and_cpu_tensors():
    from eoe_amd import explain
    from eoe_amd.models import CNN32, ClipViTB32Custom
    with pytest.raises(NotImplementedError, match="VisualTransformer"):
        explain.attention_rollout(CNN32(), torch.zeros(1, 3, 32, 32))
    vit = ClipViTB32Custom(patch_size=8, width=64, input_resolution=32, layers=1, output_dim=32)
    with pytest.raises(RuntimeError, match="GPU only"):
        explain.attention_rollout(vit, torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="fuse"):
        explain.attention_rollout(vit, torch.zeros(1, 3, 32, 32), fuse="median")
    for residual in (1.0, -0.1):
        with pytest.raises(ValueError, match="residual"):
            explain.attention_rollout(vit, torch.zeros(1, 3, 32, 32), residual=residual)
    for start in (1, -2):
        with pytest.raises(ValueError, match="start_layer"):
            explain.attention_rollout(vit, torch.zeros(1, 3, 32, 32), start_layer=start)


def test_trainer_attention_needs_extremes_and_is_off_by_default():
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    batches = [(torch.zeros(2, 3, 32, 32), torch.tensor([0, 1]))]
    ds = ListSource(batches, batches)
    with pytest.raises(ValueError, match="attention=True"):
        TRAINER["hsc"](CNN32(), dataset=ds, classes=["only"], device="cpu", attention=True)
    tr = TRAINER["hsc"](CNN32(), dataset=ds, classes=["only"], device="cpu")
    assert tr.with_attention is False and tr.attention_maps == {}
    on = TRAINER["hsc"](CNN32(), dataset=ds, classes=["only"], device="cpu", extremes=2, attention=True, explain=True)
    assert on.with_attention and on.with_explain and on.attention_maps == {}
