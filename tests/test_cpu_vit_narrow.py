"""Widths that are multiples of 64 but not of 256, without a GPU: the oracle's VisualTransformer at ViT-Ti's width against the reference's
own module (tests/golden/g28_vit_narrow.npz, written by tools/make_golden_vit_narrow.py), the argument checks of the four LayerNorm /
embed entry points, and the reference errors of the narrow case tables (tests/vit_narrow_util.py).  tests/test_gpu_vit_narrow.py holds
the HIP tower to the same fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

import rowops_util as ru
import vit_narrow_util as nu
from oracle import fill, models as omodels


def test_oracle_vit_at_width_192_reproduces_the_reference(golden):
    g = golden("g28_vit_narrow")
    geo = tuple(int(v) for v in g["geometry"])
    assert geo == nu.G28_GEOMETRY == (64, 16, 192, 2, 3, 64)
    m = omodels.deterministic_init(omodels.VisualTransformer(*geo), tag="g28", width=geo[2], layers=geo[3])
    assert m.positional_embedding.shape == (17, 192)
    x = torch.from_numpy(fill.fill("g28/x", (2, 3, geo[0], geo[0]), std=1.0))
    dy = torch.from_numpy(fill.fill("g28/dy", (2, geo[5]), std=1.0))
    out = m(x)
    (out * dy).sum().backward()
    # two fp32 evaluations of the same formulas in another order (the bars of tests/test_cpu_vit_long.py)
    assert np.abs(out.detach().numpy() - g["out"]).max() <= 1e-4 * max(1.0, np.abs(g["out"]).max())
    names = [n for n, _ in m.named_parameters()]
    assert {f"gnorm/{n}" for n in names} == {k for k in g if k.startswith("gnorm/")}
    for n, p in m.named_parameters():
        ref = float(g[f"gnorm/{n}"])
        assert abs(p.grad.double().norm().item() - ref) <= 1e-4 * ref + 1e-9, (n, ref)


@pytest.mark.parametrize("D", [100, 1088, 0, 32])
def test_layernorm_and_embed_entry_points_name_the_width_they_take(D):
    """a width that is no multiple of 64, or above 1024, is refused before any launch, and the message names the rule.  (Never called with
    a supported width here: that would launch.)"""
    from eoe_amd import _lib
    lib = _lib.lib
    assert _lib.ABI_VERSION == 5 and lib.eoe_abi_version() == 5          # no new entry point: the ABI version does not move
    buf = (C.c_float * 4096)()                                            # real host memory behind every pointer; nothing reads it
    a = C.addressof(buf)
    calls = {
        "fwd": lambda: lib.eoe_layernorm_fwd(a, max(D, 4), a, a, a, a, 1, D, 1e-5, _lib.EOE_BF16, 0, None),
        "bwd": lambda: lib.eoe_layernorm_bwd(a, 0, a, max(D, 4), a, a, None, a, max(D, 4), None, None, None, None, None, 1, D, _lib.EOE_BF16, None),
        "embed_fwd": lambda: lib.eoe_embed_lnpre_fwd(a, a, a, a, a, a, a, a, 1, 2, D, 1e-5, None),
        "embed_bwd": lambda: lib.eoe_embed_lnpre_bwd(a, a, a, a, a, a, a, a, a, None, 1, 2, D, _lib.EOE_BF16, None),
    }
    for name, call in calls.items():
        assert call() == 1, name                                          # EOE_ERR_ARG
        msg = lib.eoe_last_error()
        assert b"multiple of 64" in msg and b"1024" in msg and b"256" not in msg, (name, msg)


def test_check_vit_geometry_names_the_range_it_accepts():
    from eoe_amd.models.clip_vit import check_vit_geometry
    for width, heads in ((64, 1), (192, 3), (320, 5), (384, 6), (960, 15), (1024, 16)):
        check_vit_geometry(64, 16, width, heads)
    for width, heads in ((100, 1), (1088, 17), (96, 1)):
        with pytest.raises(NotImplementedError, match="width % 64 == 0 and width <= 1024"):
            check_vit_geometry(64, 16, width, heads)
    with pytest.raises(NotImplementedError, match="head"):
        check_vit_geometry(64, 16, 192, 4)


def test_narrow_case_tables_cover_the_listed_sizes():
    assert set(nu.LN_WIDTHS) == {64, 128, 192, 320, 384, 960, 256} and set(nu.TAIL_WIDTHS) == {64, 128, 192, 320, 384, 960}
    # every count of active tail lanes (16, 32, 48), behind zero and behind full groups
    assert {(D % 256) // 4 for D in nu.TAIL_WIDTHS} == {16, 32, 48} and {D // 256 for D in nu.TAIL_WIDTHS} == {0, 1, 3}
    assert nu.LN_ROWS == (1, 5, 9, 4100) and nu.LN_ROWS[-1] > 512 * 8
    assert set(nu.EMBED_CASES) == {(64, 1, 2), (192, 3, 17), (320, 2, 5), (384, 2, 82)}
    for geo in nu.TOWERS.values():
        assert geo["layers"] <= 2 and geo["width"] % 64 == 0 and geo["width"] % 256 != 0


def test_fp32_cpu_evaluation_of_the_narrow_cases_stays_within_the_reused_bounds():
    """the bounds the GPU tests use are rowops_util's, unchanged; the reference formula in fp32 lies inside them at every narrow case"""
    count = 0
    for what, c, specs in nu.ln_narrow_cases_all():
        ru.compare(what, c["got32"], c["ref"], specs, verbose=False)
        count += 1
    for D, n, L in nu.EMBED_CASES:
        c = ru.embed_case(D, n, L)
        ru.compare(f"embed {D} {n} {L}", c["got32"], c["ref"], ru.embed_specs(c), verbose=False)
        count += 1
    assert count == len(nu.LN_WIDTHS) * (len(nu.LN_ROWS) * 2 + 6 + 4) + len(nu.EMBED_CASES)


def test_narrow_reference_errors_are_what_the_fp32_cpu_evaluation_gives():
    """the row statistics' reference errors over the narrow tables: recorded in vit_narrow_util.NARROW_REF_ERR32 (never below the measured
    figure, not inflated past it), a little above rowops_util.REF_ERR32 and far inside the kernel bound built on the latter"""
    table = nu.measure_narrow()
    assert set(table) == set(nu.NARROW_REF_ERR32) == {"ln/mean", "ln/rstd"}
    for key, got in table.items():
        assert got <= nu.NARROW_REF_ERR32[key] <= 2.0 * got + ru.ULP32, (key, got)
        assert nu.NARROW_REF_ERR32[key] <= ru.bound_factor(key) / ru.K_KERNEL, (key, got)          # the reference itself uses under a quarter of it
