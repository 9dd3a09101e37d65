"""GPU: eoe_gemm_nt on every route of its dispatcher and eoe_gemm_tn / eoe_gemm_tn_grouped at tile edges, strides and every epilogue,
against the fp64 contract of tests/gemm_util.py (its docstring has the tables, the magnitudes and the source of every tolerance).

Every output (C, aux_out, colsum) lies in a flat buffer with PAD_ROWS canary rows in front of and behind it and canary columns in every
stride gap (fp32: a NaN-free sentinel, so that an add shows; 16 bit: a fixed bit pattern), checked bitwise after each launch; the gaps and
pad rows of every input hold NaN, so that a read at the wrong stride or past M or N poisons the result.  Every NT case asserts the route
the dispatcher took (`nt_last_kernel`), and that eoe_gemm_nt_route named it beforehand: a case that falls through to another kernel
fails.  Cases of M >= 2048 are compared with fp64 on the first and last 8 rows of every row-tile boundary plus 240 seeded rows, and over the whole tensor bitwise with the two-workgroup 160-row
kernel where test_gpu_ops.test_gemm_nt_eight_wave / test_gemm_nt_wide_kernel_tile_order_and_image establish that equality."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_util as u   # noqa: E402

SMALL_ROUTES = ("two_wg_128", "two_wg_160", "persistent_256x128", "persistent_256x96", "narrow_256x64", "persistent_narrow",
                "one_wave_160x256", "one_wave_256x256", "split_k")
BIG_ROUTES = ("eight_wave", "wide_160x256x32")
DT_IDS = lambda d: u.DTNAME[d]   # noqa: E731


@pytest.fixture(scope="module")
def ops():
    import eoe_amd.ops as o
    return o


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(mem):
    return {n: (flat.cuda(), start) for n, (flat, start) in mem.items()}


def _launch_nt(ops, c, dtype, mem, flags):
    """one launch of case c on the flat buffers `mem` (CPU; they come back with the results), with the arguments of gemm_util.nt_args:
    (route code, {'stats'}).  The route eoe_gemm_nt_route names for these arguments before the launch must be the one that ran"""
    from eoe_amd import _lib
    k, M, N = u.kind_of(c), c["M"], c["N"]
    d = _dev(mem)
    extra = {}
    addr = {n: flat.data_ptr() + start * flat.element_size() for n, (flat, start) in d.items()}
    dev = torch.device("cuda", torch.cuda.current_device())
    if k["colsum"] == "ws":                                   # the workspaces ops.gemm_nt attaches
        addr["colsum_ws"] = ops.scratch("nt_colsum_ws", (-(-M // 64) * N * 4,), torch.uint8, dev).data_ptr()
    if k["colstats"]:
        stats = torch.full((-(-M // 64), 2, N), float("nan"), dtype=torch.float32, device="cuda")
        addr["colstats_ws"] = stats.data_ptr()
    sk = ops.nt_sk_workspace(dev)
    addr["sk_ws"] = sk.data_ptr()
    args = u.nt_args(c, dtype, addr, sk.numel())
    old = _lib.set_option("nt_flags", flags)
    try:
        asked = _lib.gemm_nt_route(args, 0)
        _lib.check(_lib.lib.eoe_gemm_nt(C.byref(args), torch.cuda.current_stream().cuda_stream), "eoe_gemm_nt")
        code = _lib.get_option("nt_last_kernel")
        torch.cuda.synchronize()
    finally:
        _lib.set_option("nt_flags", old)
    assert asked == code, f"{c['id']}: eoe_gemm_nt_route said {u.NT_KERNELS[asked]}, the launch ran {u.NT_KERNELS[code]}"
    for n in ("C", "aux_out", "colsum"):
        if n in d:
            mem[n] = (d[n][0].cpu(), d[n][1])
    if k["colstats"]:
        extra["stats"] = stats.cpu()
    return code, extra


def _nt_case_failures(ops, c, dtype, rows=None):
    """everything wrong with one case: the route, the canaries, the values, repeatability of the workspace column sums"""
    k = u.kind_of(c)
    M, N = c["M"], c["N"]
    mem = u.nt_memory(c, dtype)
    code, extra = _launch_nt(ops, c, dtype, mem, c["flags"])
    if code != c["code"]:
        return [f"route: nt_last_kernel = {u.NT_KERNELS[code]}, the case is meant for {c['expect']}"]
    pair_act = None
    if c["kind"] == "gelu_nopre":
        pc = dict(c, kind="gelu")
        pm = u.nt_memory(pc, dtype)
        _launch_nt(ops, pc, dtype, pm, c["flags"])
        pair_act = u.view_of(pm["C"][0], M, N, c["ldc"], pm["C"][1])
    bad = u.nt_memory_failures(c, dtype, mem, extra, pair_act, rows)
    if k["colsum"] == "ws":                                    # partial rows added in a fixed order: the same bits twice
        again = u.nt_memory(c, dtype)
        _launch_nt(ops, c, dtype, again, c["flags"])
        for n in ("C", "colsum"):
            if not torch.equal(u.bits(again[n][0]), u.bits(mem[n][0])):
                bad.append(f"repeat:{n}: a second launch with the column-sum workspace gives other bits")
    if rows is not None and c["expect"] in BIG_ROUTES and u.fast_ok(c) and k["epi"] in ("none", "gelu", "gelu_bwd") and k["out"] == "16":
        other = u.nt_memory(c, dtype)
        code2, _ = _launch_nt(ops, c, dtype, other, u.FLAGS["two_wg_160"])
        if code2 != u.CODE["two_wg_160"]:
            bad.append(f"route: the comparison launch ran {u.NT_KERNELS[code2]}")
        for n in ("C", "aux_out"):
            if n in mem and not torch.equal(u.bits(other[n][0]), u.bits(mem[n][0])):
                bad.append(f"bitwise:{n}: differs from the two-workgroup 160-row kernel's result")
    return bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route", SMALL_ROUTES)
def test_gemm_nt_route_at_its_edges(ops, ncu, route, dtype):
    cases = u.nt_table(ncu)[route]
    assert cases
    bad = {}
    for c in cases:
        f = _nt_case_failures(ops, c, dtype)
        if f:
            bad[c["id"]] = f
    assert not bad, f"{len(bad)} of {len(cases)} cases: {bad}"


def _big_ids():
    # (the ids come from the 256-CU table; nt_table(ncu) has the same rows in the same order on any CU count -- only M of the wide route
    #  and the fall-backs' expected codes follow the count -- or, where no M qualifies for the wide route, none: those ids then skip)
    return [(r, i) for r in BIG_ROUTES for i in range(len(u.nt_table()[r]))]


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("route,index", _big_ids(), ids=lambda v: str(v))
def test_gemm_nt_heavy_route_at_its_edges(ops, ncu, route, index, dtype):
    cases = u.nt_table(ncu)[route]
    if not cases:
        pytest.skip(f"{route}: no M >= 2048 at N = 2048 fills 90 % of the 2 x {ncu} workgroup slots behind the eight-wave kernel's rule")
    assert len(cases) == len(u.nt_table()[route])
    c = cases[index]
    rows = u.case_rows(c)
    bad = _nt_case_failures(ops, c, dtype, rows)
    assert not bad, (c["id"], bad)


# ------------------------------------------------------------------------------------------------ TN
@pytest.fixture(scope="module")
def tn_ws():
    return torch.empty(512 * 256 * 128 * 4, dtype=torch.uint8, device="cuda")          # EOE_TN_WORKSPACE_BYTES


def _tn_args(ops, c, dtype, d, ws):
    from eoe_amd import _lib
    p = lambda n: d[n][0].data_ptr() + d[n][1] * d[n][0].element_size()   # noqa: E731
    return _lib.GemmArgs(p("a"), p("b"), p("C"), None, None, None, None, c["M"], c["N"], c["T"], c["lda"], c["ldb"], c["ldc"], 0,
                         ops.dtype_code(dtype), 0, 1, 1 if c["accumulate"] else 0, c["alpha"], ws.data_ptr(), ws.numel())


def _launch_tn(ops, cases, dtype, ws, tn_flags, grouped):
    from eoe_amd import _lib
    mems = [u.tn_memory(c, dtype) for c in cases]
    devs = [_dev(m) for m in mems]
    args = (_lib.GemmArgs * len(cases))(*[_tn_args(ops, c, dtype, d, ws) for c, d in zip(cases, devs)])
    st = torch.cuda.current_stream().cuda_stream
    old = _lib.set_option("tn_flags", tn_flags)
    try:
        if grouped:
            _lib.check(_lib.lib.eoe_gemm_tn_grouped(args, len(cases), st), "eoe_gemm_tn_grouped")
        else:
            _lib.check(_lib.lib.eoe_gemm_tn(C.byref(args[0]), st), "eoe_gemm_tn")
        torch.cuda.synchronize()
    finally:
        _lib.set_option("tn_flags", old)
    bad = {}
    for c, m, d in zip(cases, mems, devs):
        m["C"] = (d["C"][0].cpu(), d["C"][1])
        f = u.tn_memory_failures(c, dtype, m)
        if f:
            bad[c["id"]] = f
    return bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tn_flags", u.TN_FLAGS)
@pytest.mark.parametrize("grouped", [False, True], ids=["gemm_tn", "gemm_tn_grouped"])
def test_gemm_tn_at_its_edges(ops, tn_ws, grouped, tn_flags, dtype):
    bad = {}
    for c in u.tn_table():
        bad.update(_launch_tn(ops, [c], dtype, tn_ws, tn_flags, grouped))
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("tn_flags", u.TN_FLAGS)
def test_gemm_tn_grouped_mixes_strided_and_contiguous_problems(ops, tn_ws, tn_flags, dtype):
    bad = _launch_tn(ops, u.tn_group(), dtype, tn_ws, tn_flags, True)
    assert not bad, bad
