"""GPU tier: the ViT backward sweep outside the trainer's `zero_grad(); forward; backward` loop.  The deferred finish and the asynchronous
weight gradients write gradients after backward() has returned them; wherever autograd does not adopt the returned tensor (ops._late_write_ok)
a block must take the stream-ordered forms instead, and the sweep's state (ops._VitSweep) must survive a forward inside a live pass, a pass
that died, and a second stream.  Every case: the 4-layer tower of test_gpu_round5 (three full blocks + the class-token-only last one), 8 + 8
images, fp16, every gradient bitwise equal to the same calls under {finish per block, weight gradients in line}."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import models as omodels, trainer as otrainer  # noqa: E402

_BLOCK_VECTORS = ("ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.in_proj_bias", "attn.out_proj.bias", "mlp.c_fc.bias",
                  "mlp.c_proj.bias")


def _tower(layers):
    import eoe_amd
    from eoe_amd.models import ClipViTB32Custom
    eoe_amd.set_compute_dtype("fp16")
    return omodels.deterministic_init(ClipViTB32Custom(layers=layers), tag="r5", layers=layers).cuda().train()


@pytest.fixture(scope="module")
def model():
    """no test updates the weights, so one tower serves them all; each starts from zero_grad()"""
    return _tower(4)


@pytest.fixture(scope="module")
def batches():
    out = [tuple(t.cuda() for t in otrainer.synthetic_batch(f"r5/b{i}", 8, 8, 224)) for i in range(2)]
    torch.cuda.synchronize()
    return out


@contextlib.contextmanager
def _schedule(reference):
    from eoe_amd import ops
    old = (ops.VIT_DEFER_FINISH, ops.VIT_ASYNC_WGRAD)
    if reference:
        ops.VIT_DEFER_FINISH = ops.VIT_ASYNC_WGRAD = False
    try:
        yield
        torch.cuda.synchronize()
    finally:
        ops.VIT_DEFER_FINISH, ops.VIT_ASYNC_WGRAD = old


def _loss(m, batch):
    import eoe_amd
    return eoe_amd.hsc_loss(m(batch[0]), batch[1], 0)


def _grads(m):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in m.named_parameters()}


def _assert_same(want, got, what):
    assert want.keys() == got.keys()
    for k in want:
        if want[k] is None or got[k] is None:
            assert want[k] is None and got[k] is None, f"{what}: {k} has a gradient under one schedule only"
        else:
            assert torch.equal(want[k], got[k]), f"{what}: gradient {k} differs from the reference schedule"


def _check(scenario):
    """`scenario()` -> {name: gradients} under the reference schedule, then under the default one"""
    with _schedule(True):
        want = scenario()
    with _schedule(False):
        got = scenario()
    assert want.keys() == got.keys()
    for name in want:
        _assert_same(want[name], got[name], name)


def _counts(reset=False):
    from eoe_amd import ops
    names = ("deferred", "finished_per_block", "wgrad_async", "wgrad_inline")
    out = {k: sum(getattr(sw, k) for sw in ops._vit_sweeps.values()) for k in names}
    if reset:
        for sw in ops._vit_sweeps.values():
            sw.deferred = sw.finished_per_block = sw.wgrad_async = sw.wgrad_inline = 0
    return out


@contextlib.contextmanager
def _output_grad_hook(block, fn):
    """what a forward hook that registers a tensor hook on the block's output does (the tower calls `forward_tokens`, not the module)"""
    def forward_tokens(x2d, n, cls_only=False):
        out = type(block).forward_tokens(block, x2d, n, cls_only)
        out.register_hook(fn)
        return out
    block.forward_tokens = forward_tokens
    try:
        yield
    finally:
        del block.forward_tokens


def test_default_step_still_defers_and_overlaps(model, batches):
    """the ordinary step: p.grad is None everywhere, so all four blocks (the last one runs under the same conditions) leave their finish to
    the end-of-pass flush and their weight gradients to the side stream -- the predicate must not send this path to the fall-backs, which
    would pass every bitwise test and cost the speed"""
    from eoe_amd import ops
    assert ops.VIT_DEFER_FINISH and ops.VIT_ASYNC_WGRAD
    model.zero_grad()
    _counts(reset=True)
    _loss(model, batches[0]).backward()
    torch.cuda.synchronize()
    assert _counts() == dict(deferred=4, finished_per_block=0, wgrad_async=4, wgrad_inline=0)


def test_gradient_accumulation(model, batches):
    """two backward() calls without zero_grad: in the second every p.grad is set, autograd adds the returned tensors and frees them"""
    second = {}

    def scenario():
        model.zero_grad()
        _loss(model, batches[0]).backward()
        _counts(reset=True)
        _loss(model, batches[1]).backward()
        second.update(_counts())
        return {"accumulated": _grads(model)}

    _check(scenario)
    assert second == dict(deferred=0, finished_per_block=4, wgrad_async=0, wgrad_inline=4)      # (the default schedule ran last)


def test_one_block_in_line_between_asynchronous_ones(model, batches):
    """p.grad already set on one weight of the third block only: its weight gradients are computed in line between blocks that use the side
    stream, so its call must first order the stream behind their launches -- their buffers come round again with the next block"""
    w = model.feature_model.transformer.resblocks[2].mlp.c_fc.weight
    forms = {}

    def scenario():
        model.zero_grad()
        w.grad = torch.zeros_like(w)
        _counts(reset=True)
        _loss(model, batches[0]).backward()
        forms.update(_counts())
        return {"mixed": _grads(model)}

    _check(scenario)
    assert forms == dict(deferred=4, finished_per_block=0, wgrad_async=3, wgrad_inline=1)


def test_zero_grad_that_keeps_the_tensors(model, batches):
    def scenario():
        model.zero_grad()
        _loss(model, batches[0]).backward()
        model.zero_grad(set_to_none=False)
        _loss(model, batches[1]).backward()
        return {"second step": _grads(model)}

    _check(scenario)


def test_frozen_bias_and_layernorm(model, batches):
    """the blocks' eight vectors frozen under trainable weights: their gradients are computed and dropped at once"""
    frozen = [p for k, p in model.named_parameters() if "resblocks" in k and k.endswith(_BLOCK_VECTORS)]
    assert len(frozen) == 4 * 8

    def scenario():
        model.zero_grad()
        _loss(model, batches[0]).backward()
        return {"frozen": _grads(model)}

    for p in frozen:
        p.requires_grad_(False)
    try:
        _check(scenario)
        assert all(p.grad is None for p in frozen)
        assert all(p.grad is not None for p in model.parameters() if p.requires_grad)
    finally:
        for p in frozen:
            p.requires_grad_(True)


def test_autograd_grad_on_a_subset(model, batches):
    """autograd.grad for block 0's four weights, then an ordinary step: a stray late write of the first call would show in the second"""
    blk = model.feature_model.transformer.resblocks[0]
    weights = [blk.attn.in_proj_weight, blk.attn.out_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]

    def scenario():
        model.zero_grad()
        got = torch.autograd.grad(_loss(model, batches[0]), weights)
        subset = {str(i): g.detach().clone() for i, g in enumerate(got)}
        assert all(p.grad is None for p in model.parameters())
        _loss(model, batches[0]).backward()
        return {"subset": subset, "the step after": _grads(model)}

    _check(scenario)


def test_forward_inside_the_live_pass(model, batches):
    """a gradient hook on the second block's output scores the images with another tower while the last two blocks' finish reductions are
    queued: they must still be launched"""
    other = _tower(2)
    ran = []

    def score(_grad):
        with torch.no_grad():
            ran.append(other(batches[0][0]))

    def scenario(hooked):
        model.zero_grad()
        with _output_grad_hook(model.feature_model.transformer.resblocks[1], score) if hooked else contextlib.nullcontext():
            _loss(model, batches[0]).backward()
        return _grads(model)

    with _schedule(True):
        want = scenario(False)
    with _schedule(False):
        _assert_same(want, scenario(False), "without the hook")
        _assert_same(want, scenario(True), "with the hook")
    assert len(ran) == 1


def test_pass_that_died(model, batches):
    """a Python exception from a gradient hook on the first block's output: blocks 3, 2 and 1 have queued their work and no end-of-pass
    callback runs; the next step must neither launch nor inherit any of it"""
    def boom(_grad):
        raise RuntimeError("hook failed")

    def scenario():
        model.zero_grad()
        with _output_grad_hook(model.feature_model.transformer.resblocks[0], boom):
            with pytest.raises(RuntimeError, match="hook failed"):
                _loss(model, batches[0]).backward()
        model.zero_grad()
        _loss(model, batches[0]).backward()
        return {"the step after": _grads(model)}

    _check(scenario)


def test_two_streams(model, batches):
    """one step on the default stream, one on a fresh stream: each stream has a sweep of its own"""
    def scenario():
        model.zero_grad()
        _loss(model, batches[0]).backward()
        torch.cuda.synchronize()
        first = _grads(model)
        model.zero_grad()
        with torch.cuda.stream(torch.cuda.Stream()):
            _loss(model, batches[1]).backward()
        torch.cuda.synchronize()
        return {"default stream": first, "fresh stream": _grads(model)}

    _check(scenario)
