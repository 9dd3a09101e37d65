"""The GEMM edge suite without a GPU: the comparison functions of tests/gemm_util.py accept an fp32 restatement of eoe_gemm_nt / eoe_gemm_tn
on every case of the tables and reject every mutant by the check meant for it, the input scales keep the rounding model inside a third of
every tolerance, the docstring's figures are what the measurement gives, and the tables hold what they promise."""
import os
import re

import pytest
import torch

import gemm_util as u

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = list(u.nt_table())


@pytest.fixture(scope="module")
def measured():
    return u.measure()


@pytest.mark.parametrize("dtype", u.DTYPES, ids=lambda d: u.DTNAME[d])
@pytest.mark.parametrize("route", ROUTES)
def test_restatement_is_accepted_on_every_case(route, dtype):
    """every case of the tables in both dtypes; the M >= 2048 cases as the GPU test compares them: canaries everywhere, values on the
    sampled rows, column sums in full"""
    bad = {}
    for c in u.nt_table()[route]:
        f = u.restatement_failures(c, dtype)
        if f:
            bad[c["id"]] = f
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=lambda d: u.DTNAME[d])
def test_tn_restatement_is_accepted_on_every_case(dtype):
    bad = {c["id"]: f for c in u.tn_table() + u.tn_group() for f in [u.tn_restatement_failures(c, dtype)] if f}
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=lambda d: u.DTNAME[d])
@pytest.mark.parametrize("mutant", list(u.MUTANTS))
def test_every_mutant_is_rejected_by_the_check_meant_for_it(mutant, dtype):
    cases = u.mutant_cases()[mutant]
    assert cases
    for c in cases:
        run = u.tn_restatement_failures if mutant.startswith("tn_") else u.restatement_failures
        assert not run(c, dtype), f"{c['id']}: the unmutated restatement fails"
        found = run(c, dtype, mutant)
        assert any(f.startswith(u.MUTANTS[mutant]) for f in found), (mutant, c["id"], u.MUTANTS[mutant], found)


def test_mutant_list_is_the_issues():
    assert len(u.MUTANTS) == 18 and set(u.mutant_cases()) == set(u.MUTANTS)
    doc = u.restate32.__doc__ + u.tn_restate32.__doc__
    assert all(m in doc for m in u.MUTANTS)


def test_rounding_model_uses_at_most_a_third_of_every_tolerance(measured):
    assert measured and all(v <= 1.0 / 3.0 for v in measured.values()), measured


def test_docstring_table_is_what_the_measurement_gives(measured):
    lines = [f"    {what:56s} {v:.3f}" for what, v in sorted(measured.items())]
    doc = u.__doc__.splitlines()
    start = next(i for i, l in enumerate(doc) if l.startswith("Measured model error / allowance"))
    assert doc[start + 1:start + 1 + len(lines)] == lines, "\n".join(lines)


def _has(cases, **want):
    return any(all(c[k] == v for k, v in want.items()) for c in cases)


def test_tables_hold_the_cases_of_the_issue():
    t = u.nt_table()
    rows = {("two_wg_128", "two_wg_160"): (u.TWO_WG_M, u.TWO_WG_N, u.RING_K, u.LIST_A),
            ("persistent_256x128", "persistent_256x96"): (u.PERS_M, u.PERS_N, u.RING_K, u.LIST_A + ("colstats",)),
            ("narrow_256x64", "persistent_narrow"): (u.NARROW_M, u.NARROW_N, u.NARROW_K, u.NARROW_KINDS),
            ("one_wave_160x256", "one_wave_256x256"): (u.ONE_WAVE_M, u.ONE_WAVE_N, u.RING_K, u.LIST_A),
            ("eight_wave",): (u.W8_M, u.W8_N, u.W8_K, u.W8_KINDS), ("split_k",): (u.SPLITK_M, u.SPLITK_N, u.SPLITK_K, u.SPLITK_KINDS)}
    assert u.TWO_WG_M == (1, 63, 65, 81, 127, 129, 159, 161, 333) and u.TWO_WG_N == (72, 128, 136, 144, 264) and u.RING_K == (64, 128, 256)
    assert u.PERS_M == (1, 255, 257, 300) and u.PERS_N == (96, 104, 128, 200)
    assert u.NARROW_M == (1, 255, 257, 600) and u.NARROW_N == (8, 24, 48, 64) and u.NARROW_K == (64, 192)
    assert u.ONE_WAVE_M == (159, 161, 257, 333) and u.ONE_WAVE_N == (16, 240, 256, 272)
    assert u.W8_M == (2048, 2049, 2303, 2305) and u.W8_N == (256, 512) and u.W8_K == (128, 192, 256)
    assert u.SPLITK_M == (1, 7, 129, 1024) and u.SPLITK_N == (16, 144, 768) and u.SPLITK_K == (1536, 3072)
    for routes, (Ms, Ns, Ks, kinds) in rows.items():
        for r in routes:
            own = [c for c in t[r] if c["expect"] == r]
            for M in Ms:
                for N in Ns:
                    assert _has(own, M=M, N=N), (r, M, N)
                    assert _has(own, M=M, N=N, strides="min") and _has(own, M=M, N=N, strides="pad"), (r, M, N)
            for K in Ks:
                assert _has(own, K=K), (r, K)
            for kind in kinds:
                assert _has(own, kind=kind), (r, kind)
            assert all(c["code"] == u.CODE[c["expect"]] and c["flags"] == u.FLAGS[r] for c in t[r])
    for r in ("two_wg_128", "two_wg_160", "persistent_256x128", "persistent_256x96"):
        for kind in u.GENERIC_KINDS:
            assert any(c["kind"] == kind and not u.fast_ok(c) for c in t[r]), (r, kind)
        assert any(c["N"] % 16 for c in t[r]) and any(c["ldc"] % 8 for c in t[r]) and any(c["c_off_bytes"] == 8 for c in t[r])
    for M in (7, 130):                                      # the product's own pattern: one row in three
        assert _has(t["two_wg_128"], M=M, N=128, K=128, lda=384, ldc=384, kind="none_16_bias")
        assert _has(t["two_wg_128"], M=M, N=128, K=128, ldaux=384, ldc=384, kind="residual")
    for r in ("one_wave_160x256", "one_wave_256x256"):      # the refusal that must fall back
        assert _has(t[r], N=264, expect="two_wg_128")
    w8 = t["eight_wave"]
    for M in u.W8_M:                                        # both of its bounds depend on the strides: every (M, N) with every stride set
        for N in u.W8_N:
            assert any(c["expect"] == "eight_wave" and (c["M"], c["N"]) == (M, N) and (c["lda"], c["ldb"], c["ldc"]) == (c["K"] + 64, c["K"] + 8, N + 8)
                       for c in w8), (M, N)
            assert any(c["expect"] == "eight_wave" and (c["M"], c["N"]) == (M, N) and (c["lda"], c["ldc"]) == (c["K"] + 64, N + 64) for c in w8), (M, N)
    for kind in u.W8_REFUSED:
        assert any(c["kind"] == kind and c["expect"] != "eight_wave" for c in w8), kind
    assert any(c["K"] == 64 and c["expect"] != "eight_wave" for c in w8)
    sk = t["split_k"]
    for want in (dict(K=1472), dict(M=1025), dict(N=24)):
        assert any(all(c[k] == v for k, v in want.items()) and c["expect"] != "split_k" for c in sk), want
    assert any(c["kind"] == "residual" and c["ldaux"] > c["N"] and c["expect"] == "split_k" for c in sk)
    wide = t["wide_160x256x32"]
    assert u.wide_rows(256) == (64 * 160 - 37, 64 * 160)
    assert all(c["expect"] == "wide_160x256x32" and c["N"] == 2048 for c in wide)
    for kind in u.LIST_A:
        assert _has(wide, kind=kind), kind
    assert {c["K"] for c in wide} == {64, 256} and {c["M"] for c in wide} == {10203, 10240}
    for kind in u.GENERIC_KINDS:                            # each kind once through epilogue_generic, on the ragged M
        assert any(c["kind"] == kind and not u.fast_ok(c) and c["M"] == 10203 for c in wide), kind
    assert any(c["ldc"] % 8 for c in wide) and any(c["c_off_bytes"] == 8 for c in wide)
    assert any(c["kind"] == "gelu" and c["ldc"] % 8 for c in wide) and any(c["kind"] == "gelu" and c["c_off_bytes"] == 8 for c in wide)
    tn = u.tn_table()
    for T in (1, 63, 64, 65, 200):
        for M, N in ((8, 8), (136, 264), (256, 128)):
            for s in ("min", "pad"):
                assert _has(tn, T=T, M=M, N=N, strides=s, accumulate=False) and _has(tn, T=T, M=M, N=N, strides=s, accumulate=True, alpha=0.5)
    assert _has(tn, strides="pad", lda=136 + 8, ldb=3 * 264, ldc=264 + 4)
    assert {c["strides"] for c in u.tn_group()} == {"min", "pad"}


def test_no_kind_or_k_is_tied_to_one_n():
    t = u.nt_table()
    for r, Ns, kinds in (("two_wg_128", u.TWO_WG_N, u.LIST_A), ("two_wg_160", u.TWO_WG_N, u.LIST_A), ("persistent_256x128", u.PERS_N, u.LIST_A),
                         ("persistent_256x96", u.PERS_N, u.LIST_A), ("narrow_256x64", u.NARROW_N, u.NARROW_KINDS),
                         ("persistent_narrow", u.NARROW_N, u.NARROW_KINDS), ("one_wave_160x256", u.ONE_WAVE_N, u.LIST_A),
                         ("one_wave_256x256", u.ONE_WAVE_N, u.LIST_A), ("eight_wave", u.W8_N, u.W8_KINDS), ("split_k", u.SPLITK_N, u.SPLITK_KINDS)):
        own = [c for c in t[r] if c["expect"] == r]
        for kind in kinds:
            assert len({c["N"] for c in own if c["kind"] == kind}) >= 2, (r, kind)
            assert len({c["K"] for c in own if c["kind"] == kind}) >= 2, (r, kind)
        for N in Ns:
            assert len({c["K"] for c in own if c["N"] == N}) >= 2, (r, N)


def test_wide_route_rows_follow_the_cu_count():
    for ncu in (64, 104, 228, 256, 304):
        Ms = u.wide_rows(ncu)
        assert Ms and Ms[0] >= 2048 and Ms[1] % 160 == 0 and Ms[0] == Ms[1] - 37
        assert all(c["expect"] == "wide_160x256x32" for c in u.nt_table(ncu)["wide_160x256x32"])


def _route(args, ncu, flags):
    """the name of the route eoe_gemm_nt_route gives under nt_flags = flags (restored afterwards)"""
    from eoe_amd import _lib
    old = _lib.set_option("nt_flags", flags)
    try:
        return u.NT_KERNELS[_lib.gemm_nt_route(args, ncu)]
    finally:
        _lib.set_option("nt_flags", old)


@pytest.mark.parametrize("ncu", (64, 104, 228, 256, 304))
def test_route_query_gives_the_tables_route_on_every_cu_count(ncu):
    """the product's rule (nt_route of gemm.hip, asked through eoe_gemm_nt_route: no GPU, nothing launched) against gemm_util.dispatch on
    every row of the tables, with the arguments the GPU test launches with"""
    bad = {}
    for cases in u.nt_table(ncu).values():
        for c in cases:
            for dt in u.DTYPES:
                got = _route(u.nt_args(c, dt, u.fake_addresses(c, dt), u.sk_workspace_bytes(ncu)), ncu, c["flags"])
                if got != c["expect"]:
                    bad[f"{c['id']}-{u.DTNAME[dt]}"] = (got, c["expect"])
    assert not bad, f"{len(bad)} rows: {bad}"


def test_fake_addresses_lie_where_the_gpu_tests_views_lie():
    for route in ("two_wg_128", "persistent_256x96", "narrow_256x64", "one_wave_160x256"):
        for c in u.nt_table()[route]:
            for dt in u.DTYPES:
                mem, st = u.nt_memory(c, dt), u.nt_starts(c, dt)
                assert {n: (start, flat.element_size()) for n, (flat, start) in mem.items()} == st, c["id"]
                assert all(a % 16 == (st[n][0] * st[n][1]) % 16 for n, a in u.fake_addresses(c, dt).items() if n in st)


def test_route_query_stream_k_needs_a_usable_workspace():
    """test_gpu_round5.test_streamk_and_splitk_fall_back_without_a_usable_workspace's shape, eight-wave kernel forced, stream-K asked for, on
    256 CUs: the stream-K form only with a whole, aligned workspace"""
    c = u.nt_case("eight_wave", "none_16", 4096, 2304, 768, flags=1 | 262144 | 1048576)
    full = u.sk_workspace_bytes(256)

    def route(sk_ws, nbytes):
        return _route(u.nt_args(c, torch.float16, dict(u.fake_addresses(c, torch.float16), sk_ws=sk_ws), nbytes), 256, c["flags"])

    ws = u.fake_addresses(c, torch.float16)["sk_ws"]
    assert ws % 16 == 0 and route(ws, full) == "eight_wave_stream_k"
    assert route(None, 0) == "eight_wave" and route(ws, full - 1) == "eight_wave" and route(ws + 8, full) == "eight_wave"


@pytest.mark.parametrize("mode", ("one_tap_per_k_tile", "packed_first_layer", "narrow_channels"))
def test_route_query_gather_forms(mode):
    """one implicit-convolution call per gather mode (1, 2, and 1 with 8 channels, which eoe_gemm_nt decodes as mode 3) at the smallest
    geometry the argument checks accept: one output pixel of one image, one 64-deep k-tile"""
    from eoe_amd import _lib
    C_, W, stride, gather = {"one_tap_per_k_tile": (64, 1, 1, 1), "packed_first_layer": (4, 8, 2, 2), "narrow_channels": (8, 1, 1, 1)}[mode]
    c = u.nt_case("narrow_256x64", "none_f32", 1, 8, 64)
    g = u.nt_args(c, torch.bfloat16, u.fake_addresses(c, torch.bfloat16), 0)
    g.gather, g.geo = gather, _lib.ConvGeometry(n=1, H=1, W=W, C=C_, kh=1, kw=1, stride=stride, pad=0, Ho=1, Wo=1)
    for ncu in (64, 256):
        assert _route(g, ncu, 1) == "gather"


def test_route_query_flag_64_sends_narrow_n_to_the_persistent_kernel():
    c = u.nt_case("persistent_narrow", "none_f32", 257, 48, 64, flags=1 | 64)
    g = u.nt_args(c, torch.bfloat16, u.fake_addresses(c, torch.bfloat16), 0)
    assert _route(g, 256, 1 | 64) == "persistent_narrow" and _route(g, 256, 1) == "narrow_256x64"


def test_route_query_checks_its_arguments_like_the_launch():
    from eoe_amd import _lib
    c = u.nt_case("two_wg_128", "none_f32", 65, 72, 64)
    g = u.nt_args(c, torch.bfloat16, u.fake_addresses(c, torch.bfloat16), 0)
    g.K = 65
    with pytest.raises(_lib.EoeError, match="multiple of 64"):
        _lib.gemm_nt_route(g, 256)


def test_inputs_are_16_bit_values_and_pure_functions_of_their_name():
    c = u.nt_table()["two_wg_128"][3]
    for dt in u.DTYPES:
        x = u.nt_inputs(c, dt)
        assert x["a"].dtype == dt and x["b"].dtype == dt
        u._nt_inputs.cache_clear()
        y = u.nt_inputs(c, dt)
        assert all(torch.equal(u.bits(x[n]), u.bits(y[n])) for n in x if x[n] is not None)
        again = u.r16(f"gemm/nt/{u.DTNAME[dt]}/{u.kind_of(c)['epi']}/{c['M']}x{c['N']}x{c['K']}/a", (c["M"], c["K"]), u.A_STD, dt)
        assert torch.equal(u.bits(again), u.bits(x["a"]))
        t = u.tn_inputs(u.tn_table()[5], dt)
        assert t["a"].dtype == dt and torch.equal(u.bits(t["a"]), u.bits(u.tn_inputs(u.tn_table()[5], dt)["a"]))


def test_route_codes_mirror_the_header():
    from_header = re.findall(r"EOE_NT_KERNEL_(\w+) = (\d+)", open(os.path.join(ROOT, "include", "eoe_hip.h")).read())
    assert [n.lower() for n, _ in from_header] == list(u.NT_KERNELS) and [int(v) for _, v in from_header] == list(range(len(u.NT_KERNELS)))
    src = open(os.path.join(ROOT, "eoe_amd", "_lib.py")).read()
    mirror = re.search(r"NT_KERNELS = \((.*?)\)", src, re.S).group(1)
    assert re.findall(r'"(\w+)"', mirror) == list(u.NT_KERNELS)


def test_canaries_notice_a_stray_write_and_an_add():
    flat, start = u.canary(100, torch.float32), 20
    assert not u.canary_failures(flat, 4, 6, 10, start, "C")
    flat[start + 7] += 1.0                                   # a gap column
    assert u.canary_failures(flat, 4, 6, 10, start, "C")
    f16 = u.canary(100, torch.bfloat16)
    f16[3] = 0.0
    assert u.canary_failures(f16, 4, 6, 10, start, "C") and bool(torch.isfinite(u.canary(4, torch.float16).float()).all())
