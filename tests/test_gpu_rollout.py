"""GPU: attention rollout (csrc/rollout.hip, eoe_amd/explain.py).  eoe_attn_probs against the float64 statement at every length edge, head
count, magnitude and fuse mode; eoe_rollout_step and eoe_rollout_map against float64 / numpy; attention_rollout end to end against a
float64 restatement of the tower; the trainer option.  Case tables and the bars with their measurements: tests/rollout_util.py."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rollout_util as ru                                         # noqa: E402


@pytest.fixture(autouse=True)
def _restore():
    import eoe_amd
    old = eoe_amd.compute_dtype()
    yield
    eoe_amd.set_compute_dtype(old)


def guarded(shape):
    """an fp32 output tensor with ru.GUARD elements of NaN behind it: (the view to write, the guard)"""
    n = int(np.prod(shape))
    buf = torch.full((n + ru.GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    return buf[:n].view(shape), buf[n:]


def probs_dev(qkv, n, L, heads, fuse):
    from eoe_amd import explain, ops
    from eoe_amd._lib import check, lib
    out, guard = guarded((n, L, L))
    check(lib.eoe_attn_probs(qkv.data_ptr(), out.data_ptr(), n, L, heads, ops.dtype_code(qkv.dtype), explain.FUSE[fuse], ops._stream()),
          "eoe_attn_probs")
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all()), "eoe_attn_probs wrote behind its output"
    return out


def step_dev(probs, r_in, residual):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    n, L, _ = probs.shape
    out, guard = guarded((n, L, L))
    check(lib.eoe_rollout_step(probs.data_ptr(), ops._p(r_in), out.data_ptr(), n, L, residual, ops._stream()), "eoe_rollout_step")
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all()), "eoe_rollout_step wrote behind its output"
    return out


# ------------------------------------------------------------------------------------------------ probabilities
@pytest.mark.parametrize("L,heads,n", ru.PROBS_CASES)
def test_attn_probs_against_the_float64_statement(L, heads, n):
    """bar ru.PROBS_BAR = 2.3e-5 = 4 x 5.75e-6, the largest error of the fp32 numpy restatement against float64 on these inputs
    (rollout_util); rows of the mean fuse sum to one within bar x L; one head: the three fuse modes are the same bits; two runs are the
    same bits; nothing is written behind the output"""
    from eoe_amd.explain import attention_probs_np
    worst = 0.0
    for dt in ru.DTYPES:
        for kind in ru.KINDS:
            q = ru.qkv_case(L, heads, n, dt, kind)
            qd = q.cuda()
            got = {}
            for fuse in ru.FUSES:
                got[fuse] = probs_dev(qd, n, L, heads, fuse)
                assert torch.equal(got[fuse], probs_dev(qd, n, L, heads, fuse)), (dt, kind, fuse, "two runs differ")
                ref = attention_probs_np(q.float().numpy(), n, L, heads, fuse)
                g = got[fuse].cpu().numpy().astype(np.float64)
                assert np.isfinite(g).all(), (dt, kind, fuse)
                err = np.abs(g - ref).max()
                worst = max(worst, err)
                assert err <= ru.PROBS_BAR, (dt, kind, fuse, err)
            sums = got["mean"].double().sum(dim=2)
            assert float((sums - 1).abs().max()) <= ru.PROBS_BAR * L, (dt, kind)
            if heads == 1:
                assert torch.equal(got["mean"], got["max"]) and torch.equal(got["mean"], got["min"]), (dt, kind)
            if kind == "equal":
                assert float((got["mean"] - 1.0 / L).abs().max()) <= ru.PROBS_BAR
    print(f"attn_probs L={L} heads={heads} n={n}: worst |error| {worst:.3e} (bar {ru.PROBS_BAR:.3e})")


@pytest.mark.parametrize("L", (50, 197))
@pytest.mark.parametrize("dtype", ru.DTYPES)
def test_attn_probs_finds_a_planted_key(L, dtype):
    """the key of token j is twice query 0 in every head: query 0's logit for it is 16 against unit-scale others"""
    heads, n, j = 12, 3, L - 7
    D = 64 * heads
    q = ru.qkv_case(L, heads, n, torch.float32, "gauss").reshape(n, L, 3 * D)
    q[:, j, D:2 * D] = 2.0 * q[:, 0, :D]
    qd = q.reshape(n * L, 3 * D).to(dtype).cuda()
    for fuse in ru.FUSES:
        p = probs_dev(qd, n, L, heads, fuse)
        assert bool((p[:, 0, j] > 0.99).all()) and bool((p[:, 0].argmax(dim=1) == j).all()), (fuse, p[:, 0, j])


# ------------------------------------------------------------------------------------------------ the step and the map
@pytest.mark.parametrize("L,n", ru.STEP_CASES)
def test_rollout_step_against_float64(L, n):
    """bar ru.STEP_BAR = 1.24e-5 = 4 x 3.1e-6, the largest error of the fp32 numpy chain against float64 on these inputs (rollout_util),
    after one and after four steps; every R's rows sum to one within bar x L; r_in = NULL is an explicit identity bit for bit"""
    worst = 0.0
    eye = torch.eye(L, device="cuda").expand(n, L, L).contiguous()
    for residual in ru.RESIDUALS:
        for kind in ru.STEP_KINDS:
            chain = ru.step_chain_case(L, n, kind)
            ref = ru.rollout_chain_np(chain, residual, np.float64)
            dev = [torch.from_numpy(p).cuda() for p in chain]
            r = step_dev(dev[0], None, residual)
            assert torch.equal(r, step_dev(dev[0], eye, residual)), (residual, kind, "NULL is not the identity")
            assert torch.equal(r, step_dev(dev[0], None, residual)), (residual, kind, "two runs differ")
            for s in range(4):
                if s:
                    r = step_dev(dev[s], r, residual)
                if s in (0, 3):
                    g = r.cpu().numpy().astype(np.float64)
                    err = np.abs(g - ref[s]).max()
                    worst = max(worst, err)
                    assert err <= ru.STEP_BAR, (residual, kind, s, err)
                    assert np.abs(g.sum(axis=2) - 1).max() <= ru.STEP_BAR * L, (residual, kind, s)
    print(f"rollout_step L={L} n={n}: worst |error| {worst:.3e} (bar {ru.STEP_BAR:.3e})")


def test_rollout_step_takes_a_zero_or_non_finite_row_as_the_identity_row():
    L = 50
    p = torch.from_numpy(ru.step_probs_case(L, 2, "stochastic")).cuda()
    p[0, 3] = 0.0
    p[1, 49] = 0.0
    p[1, 7, 5] = float("nan")
    p[0, 20, 1] = float("inf")
    r = step_dev(p, None, 0.0)
    eye = torch.eye(L, device="cuda")
    for img, row in ((0, 3), (1, 49), (1, 7), (0, 20)):
        assert torch.equal(r[img, row], eye[row]), (img, row)
    assert bool(torch.isfinite(r).all())
    # with a residual a zero row of probs is the identity row by arithmetic: residual / residual
    r = step_dev(p, None, 0.5)
    assert torch.equal(r[0, 3], eye[3]) and torch.equal(r[1, 7], eye[7])


@pytest.mark.parametrize("grid,patch", ru.MAP_CASES)
def test_rollout_map_is_the_class_row_repeated_over_the_patches(grid, patch):
    from eoe_amd import ops
    from eoe_amd._lib import check, lib
    n, L = 3, grid * grid + 1
    r = torch.randn((n, L, L), generator=ru._gen("map", grid, patch))
    out, guard = guarded((n, grid * patch, grid * patch))
    check(lib.eoe_rollout_map(r.cuda().data_ptr(), out.data_ptr(), n, L, grid, patch, ops._stream()), "eoe_rollout_map")
    torch.cuda.synchronize()
    assert bool(torch.isnan(guard).all())
    want = np.repeat(np.repeat(r[:, 0, 1:].reshape(n, grid, grid).numpy(), patch, axis=1), patch, axis=2)
    assert np.array_equal(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ end to end
NORM = ((0.5, 0.4, 0.45), (0.25, 0.3, 0.2))


def make_tower(name):
    from eoe_amd.models import ClipViTB32Custom
    kw = ru.TOWERS[name][0]
    torch.manual_seed(11)
    m = ClipViTB32Custom(**kw)
    with torch.no_grad():
        for blk in m.feature_model.transformer.resblocks:
            blk.attn.in_proj_weight.mul_(2.0)            # sharper attention than xavier's near-uniform rows
    return m


@pytest.fixture(scope="module")
def tower_refs():
    """per tower: (model on the CPU, images, float64 maps) -- computed once, shared, left unchanged"""
    out = {}
    for name, (kw, res, patch, heads) in ru.TOWERS.items():
        m = make_tower(name)
        imgs = ru.tower_images(name)
        maps, _ = ru.tower_rollout_f64(m.state_dict(), imgs, patch, heads, kw["layers"], normalize=NORM)
        out[name] = (m, imgs, maps)
    return out


@pytest.mark.parametrize("name", list(ru.TOWERS))
@pytest.mark.parametrize("dtype", ru.DTYPES)
def test_attention_rollout_against_the_float64_tower(tower_refs, name, dtype):
    """bar = 4 x the largest map error of the float64 restatement with each layer's qkv rounded to the compute type against the pure
    float64 run (measured here on the CPU, printed); the maps are constant on every patch block, non-negative and finite; the model's
    parameters, .grad fields and train / eval flags are untouched.  Measured (emulation -> bar; attention_rollout on an MI355X):
    b32 fp16 1.07e-5 -> 4.28e-5; 1.63e-5.  b32 bf16 6.26e-5 -> 2.50e-4; 2.20e-4.  narrow65 fp16 4.58e-5 -> 1.83e-4; 9.40e-5.
    narrow65 bf16 2.73e-4 -> 1.09e-3; 9.66e-4."""
    import eoe_amd
    from eoe_amd import explain
    kw, res, patch, heads = ru.TOWERS[name]
    m0, imgs, ref = tower_refs[name]
    emu, _ = ru.tower_rollout_f64(m0.state_dict(), imgs, patch, heads, kw["layers"], normalize=NORM, round_qkv=dtype)
    measured = np.abs(emu - ref).max()
    bar = 4 * measured
    eoe_amd.set_compute_dtype(dtype)
    m = copy.deepcopy(m0).cuda().train()
    m.feature_model.set_normalize(*NORM)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flags = [mod.training for mod in m.modules()]
    maps = explain.attention_rollout(m, imgs.cuda())
    torch.cuda.synchronize()
    assert maps.shape == (4, res, res) and maps.dtype == torch.float32 and maps.is_cuda
    assert bool(torch.isfinite(maps).all()) and float(maps.min()) >= 0.0
    g = res // patch
    blocks = maps.reshape(4, g, patch, g, patch)
    assert torch.equal(blocks, blocks[:, :, :1, :, :1].expand_as(blocks))
    err = np.abs(maps.cpu().numpy().astype(np.float64) - ref).max()
    print(f"attention_rollout {name} {dtype}: |error| {err:.3e}, qkv-rounding emulation {measured:.3e}, bar {bar:.3e}, map scale {ref.max():.3e}")
    assert err <= bar, (err, bar)
    assert torch.equal(maps, explain.attention_rollout(m, imgs.cuda()))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert all(p.grad is None for p in m.parameters()) and flags == [mod.training for mod in m.modules()]


@pytest.mark.parametrize("name", list(ru.TOWERS))
def test_last_layer_without_residual_is_the_raw_class_token_attention(tower_refs, name):
    """start_layer = -1, residual = 0 against row 0 of the last block's attention_probs, bit for bit: the fp32 sum of a softmax row
    is one within its own rounding, which eoe_rollout_step takes as one (2^-20), so the step leaves such a row its bits"""
    import eoe_amd
    from eoe_amd import explain
    kw, res, patch, heads = ru.TOWERS[name]
    eoe_amd.set_compute_dtype(torch.float16)
    m = copy.deepcopy(tower_refs[name][0]).cuda().eval()
    imgs = tower_refs[name][1].cuda()
    maps = explain.attention_rollout(m, imgs, start_layer=-1, residual=0.0)
    vit = m.feature_model
    blocks = list(vit.transformer.resblocks)
    g = res // patch
    L = g * g + 1
    with torch.no_grad():
        tok = vit.embed(imgs)
        for blk in blocks[:-1]:
            tok = blk.forward_tokens(tok, 4)
        probs = explain.attention_probs(explain.block_qkv(blocks[-1], tok), 4, L, heads)
    want = probs[:, 0, 1:].reshape(4, g, 1, g, 1).expand(4, g, patch, g, patch).reshape(4, res, res)
    diff = (maps - want).abs().max().item()
    print(f"raw class-token attention {name}: largest |difference| {diff:.3e} at a map scale of {want.max().item():.3e}")
    assert torch.equal(maps, want), diff


# ------------------------------------------------------------------------------------------------ trainer
@pytest.fixture(scope="module")
def small_task():
    """a resident 32-px set and a one-block ViT-Ti tower (17 tokens, 3 heads), trained for one epoch"""
    import eoe_amd
    from eoe_amd.data import ResidentImageSource
    from eoe_amd.models import ClipViTB32Custom
    from eoe_amd.training import TRAINER
    old = eoe_amd.compute_dtype()
    eoe_amd.set_compute_dtype("bf16")
    g = torch.Generator().manual_seed(7)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 32), torch.linspace(0, 1, 32), indexing="ij")

    def make(k, n):
        pat = torch.stack([torch.sin(6.28 * (k + 1) * xx), torch.cos(6.28 * (k + 1) * yy), torch.sin(6.28 * (xx + yy) * (k + 1))], -1)
        return (128 + 60 * pat.unsqueeze(0) + 25 * torch.randn((n, 32, 32, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    test_y = torch.tensor([0, 1] * 8)
    test = torch.stack([make(int(y), 1)[0] for y in test_y])
    ds = ResidentImageSource(make(0, 32), make(1, 32), test, test_y, crop=32, mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), seed=3)
    torch.manual_seed(0)
    m0 = ClipViTB32Custom(width=192, layers=1, input_resolution=32, patch_size=8, output_dim=64)
    tr = TRAINER["hsc"](m0, dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"])
    model, _ = tr.train_cls(copy.deepcopy(m0), ds, 0, "only", 0)
    eoe_amd.set_compute_dtype(old)
    return ds, m0, model


def test_trainer_rolls_out_its_extremes_and_changes_nothing_when_off(small_task, tmp_path):
    import eoe_amd
    from eoe_amd import explain
    from eoe_amd.training import TRAINER
    from eoe_amd.training.ad_trainer import JsonLogger

    class Keeping(JsonLogger):
        def logimg(self, name, *a, **k):
            self.pictures = getattr(self, "pictures", {})
            self.pictures[name] = super().logimg(name, *a, **k)
            return self.pictures[name]
    eoe_amd.set_compute_dtype("bf16")
    ds, m0, model = small_task
    kw = dict(dataset=ds, epochs=1, lr=1e-4, wdk=1e-3, milestones=[], batch_size=16, classes=["only"], extremes=2)
    on = TRAINER["hsc"](m0, logger=Keeping(str(tmp_path / "on")), attention=True, **kw)
    off = TRAINER["hsc"](m0, logger=JsonLogger(str(tmp_path / "off")), **kw)
    roc_on, prc_on = on.eval_cls(model, ds, 0, "only", 0)
    roc_off, prc_off = off.eval_cls(model, ds, 0, "only", 0)
    key = "eval_cls0_it0"
    assert list(on.attention_maps) == [key] and off.attention_maps == {} and on.explanations == {}
    assert roc_on.auc == roc_off.auc and prc_on.avg_prec == prc_off.avg_prec
    assert on.extremes[key].as_dict() == off.extremes[key].as_dict()
    files = {d: sorted(os.listdir(tmp_path / d)) for d in ("on", "off")}
    extra = sorted(set(files["on"]) - set(files["off"]))
    assert set(files["off"]) <= set(files["on"]) and extra and all(f.startswith("eval_cls0-only_it0_extremes_attn") for f in extra), files
    for f in files["off"]:
        if os.path.isfile(tmp_path / "off" / f):
            assert (tmp_path / "off" / f).read_bytes() == (tmp_path / "on" / f).read_bytes(), f
    got = on.logger.pictures["eval_cls0-only_it0_extremes_attn"]
    assert got.ndim == 3 and got.shape[2] == 3 and got.std() > 10
    # the maps, recomputed by hand for the same rows
    rows, per, _ = on._extreme_rows(on.extremes[key])
    maps = on.attention_maps[key]
    assert per == 2 and maps.shape == (len(rows), 32, 32) and maps.dtype == torch.float32 and bool(torch.isfinite(maps).all())
    model = model.cuda()
    assert torch.equal(explain.attention_rollout(model, ds.test_inputs(rows)[0].cuda()), maps)
    model.cpu()
    # run() starts with an empty dictionary
    on.attention_maps["stale"] = maps
    on.run(run_classes=[0], train=False, test=False)
    assert on.attention_maps == {}


def test_trainer_attention_refuses_before_scoring(small_task):
    from eoe_amd.data import ListSource
    from eoe_amd.models import CNN32
    from eoe_amd.training import TRAINER
    ds, m0, model = small_task
    batches = [(torch.zeros(2, 3, 32, 32), torch.tensor([0, 1]))]

    class Counting(ListSource):
        asked = 0

        def loaders(self, *a, **k):
            Counting.asked += 1
            return super().loaders(*a, **k)
    tr = TRAINER["hsc"](m0, dataset=Counting(batches, batches), classes=["only"], extremes=2, attention=True)
    with pytest.raises(NotImplementedError, match=r"attention=True needs a source with test_inputs"):
        tr.eval_cls(model, tr.ds, 0, "only", 0)
    assert Counting.asked == 0
    cnn = TRAINER["hsc"](CNN32(), dataset=ds, classes=["only"], extremes=2, attention=True)
    with pytest.raises(NotImplementedError, match=r"attention=True needs a ViT encoder"):
        cnn.eval_cls(CNN32(), ds, 0, "only", 0)
