"""GPU: the implicit patch matrices of eoe_gemm_nt and eoe_gemm_tn_grouped and the data-movement entry points of csrc/conv.hip, each alone,
BITWISE against the integer references of tests/conv_gather_util.py (its docstring has the tables, the exactness condition and the
identity probe).  Every output lies in canaries that are checked after each launch, every launch is synchronised before the next, every
NT case asserts the kernel that ran (`nt_last_kernel` = gather and `nt_last_form` = mi 16 + ni).  Nothing here is a measured number.
The identity probe of mode 2 is compared with the unfold alone: eoe_im2col takes no 4-channel NHWC tensor."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import conv_gather_util as u   # noqa: E402
import gemm_util as gu   # noqa: E402

DT_IDS = lambda d: u.DTNAME[d]   # noqa: E731
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from eoe_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dcode(lib, dtype):
    return {torch.float16: lib.EOE_F16, torch.bfloat16: lib.EOE_BF16}[dtype]


def _dev(mem):
    return {n: (flat.cuda(), start) for n, (flat, start) in mem.items()}


def _addr(d):
    return {n: flat.data_ptr() + start * flat.element_size() for n, (flat, start) in d.items()}


def _run_nt(lib, c, args):
    """one synchronised launch under the case's nt_flags: what is wrong with the route, or []"""
    old = lib.set_option("nt_flags", c["flags"])
    try:
        asked = lib.gemm_nt_route(args, 0)
        lib.check(lib.lib.eoe_gemm_nt(C.byref(args), _stream()), "eoe_gemm_nt")
        code, form = lib.get_option("nt_last_kernel"), lib.get_option("nt_last_form")
        torch.cuda.synchronize()
    finally:
        lib.set_option("nt_flags", old)
    if (asked, code, form) != (lib.NT_KERNEL_GATHER, lib.NT_KERNEL_GATHER, c["form"]):
        return [f"route: asked {asked}, ran {code} with nt_last_form {form}; the case is for {c['expect']} (form {c['form']})"]
    return []


def _nt_case_failures(lib, c, dtype, rows=None):
    k = u.kind_of(c)
    mem = u.nt_memory(c, dtype)
    d = _dev(mem)
    addr = _addr(d)
    stats = None
    if k["colstats"]:
        stats = torch.full((u.cdiv(c["M"], 64), 2, c["N"]), NAN, dtype=torch.float32, device="cuda")
        addr["colstats_ws"] = stats.data_ptr()
    bad = _run_nt(lib, c, u.nt_args(c, dtype, addr))
    if bad:
        return bad
    mem["C"] = (d["C"][0].cpu(), d["C"][1])
    return u.nt_failures(c, dtype, mem, None if stats is None else stats.cpu(), rows)


def _im2col16(lib, x16, gg, Cc, Kp, dtype):
    """eoe_im2col of a 16-bit NHWC tensor on the device -> [M, Kp]"""
    out = torch.full((gg["n"] * gg["Ho"] * gg["Wo"], Kp), NAN, dtype=dtype, device="cuda")
    lib.check(lib.lib.eoe_im2col(x16.data_ptr(), 0, None, None, out.data_ptr(), gg["n"], Cc, gg["H"], gg["W"], gg["kh"], gg["kw"], gg["s"],
                                 gg["p"], Kp, _dcode(lib, dtype), _stream()), "eoe_im2col")
    torch.cuda.synchronize()
    return out


def _nt_probe_failures(lib, c, dtype):
    """the implicit patch matrix read out through one-hot weights, window by window: bitwise the unfold and eoe_im2col's output"""
    x = u.probe_activation(c)
    want = torch.from_numpy(u.nt_patch(c, x).astype(np.float32)).cuda()
    a = u.t16(x, dtype).cuda()
    bad = []
    if c["mode"] != 2:
        col = _im2col16(lib, a, c["gg"], c["C"], c["K"], dtype)
        if not torch.equal(col.float(), want):
            bad.append("probe: eoe_im2col differs from the unfold")
    N = c["N"]
    for k0 in u.probe_windows(c, N):
        b = u.probe_b(c, k0, N, dtype).cuda()
        out = torch.full((c["M"], N), NAN, dtype=torch.float32, device="cuda")
        args = u.nt_args(dict(c, ldb=c["K"]), dtype, {"a": a.data_ptr(), "b": b.data_ptr(), "C": out.data_ptr()}, out_f32=True, plain=True)
        bad += _run_nt(lib, c, args)
        w = min(N, c["K"] - k0)
        if not torch.equal(out[:, :w], want[:, k0:k0 + w]) or bool((out[:, w:] != 0).any()):
            ne = (out[:, :w] != want[:, k0:k0 + w]).nonzero()
            i, j = (int(v) for v in ne[0]) if len(ne) else (-1, -1)
            bad.append(f"probe: columns {k0}..{k0 + w}: {len(ne)} elements of the patch matrix differ, first at row {i}, column {k0 + j}: "
                       f"{float(out[i, j])} for {float(want[i, k0 + j])}")
        if len(bad) > 3:
            break
    return bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kernel", [k for k in u.KERNELS if any(not c["heavy"] for c in u.nt_table()[k])])
def test_gemm_nt_gather_kernel_at_its_edges(lib, ncu, kernel, dtype):
    cases = [c for c in u.nt_table(ncu)[kernel] if not c["heavy"]]
    assert cases
    bad = {}
    for c in cases:
        assert c["expect"] == kernel, c["id"]
        f = _nt_case_failures(lib, c, dtype)
        if f:
            bad[c["id"]] = f
    assert not bad, f"{len(bad)} of {len(cases)} cases: {bad}"


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kernel", [k for k in u.KERNELS if any(not c["heavy"] for c in u.nt_table()[k])])
def test_gemm_nt_gather_identity_probe(lib, ncu, kernel, dtype):
    bad = {}
    for c in [c for c in u.nt_table(ncu)[kernel] if not c["heavy"]]:
        f = _nt_probe_failures(lib, c, dtype)
        if f:
            bad[c["id"]] = f
    assert not bad, bad


def _heavy_ids():
    return [(k, i) for k, cs in u.nt_table().items() for i, c in enumerate(cs) if c["heavy"]]


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("kernel,index", _heavy_ids(), ids=lambda v: str(v))
def test_gemm_nt_gather_second_tile_and_160_row_cases(lib, ncu, kernel, index, dtype):
    """the persistent kernel's second tile per workgroup (modes 1, 2, 3: the tap cursor restarts) and the 160-row two-workgroup kernel,
    sized from the CU count; compared on the first and last 8 rows of every row tile plus 240 seeded rows"""
    c = u.nt_table(ncu)[kernel][index]
    assert c["heavy"]
    if c["expect"] != kernel:
        pytest.skip(f"{kernel}: on {ncu} CUs this shape takes {c['expect']}")
    if kernel.startswith("pers"):
        assert u.cdiv(c["M"], 256) * u.cdiv(c["N"], 128) > ncu
    bad = _nt_case_failures(lib, c, dtype, u.case_rows(c))
    assert not bad, (c["id"], bad)


# ------------------------------------------------------------------------------------------------ TN
@pytest.fixture(scope="module")
def tn_ws():
    return torch.empty(512 * 256 * 128 * 4, dtype=torch.uint8, device="cuda")          # EOE_TN_WORKSPACE_BYTES


def _run_tn(lib, args):
    lib.check(lib.lib.eoe_gemm_tn_grouped(C.byref(args), 1, _stream()), "eoe_gemm_tn_grouped")
    torch.cuda.synchronize()


def _tn_case_failures(lib, c, dtype, ws, ncu):
    mem = u.tn_memory(c, dtype)
    d = _dev(mem)
    _run_tn(lib, u.tn_args(c, dtype, _addr(d), ws.data_ptr(), ws.numel()))
    mem["C"] = (d["C"][0].cpu(), d["C"][1])
    return u.tn_failures(c, mem, ncu)


def _tn_probe_failures(lib, c, dtype, ws):
    """dy = unit vectors: column j of the output is row t0 + j of the implicit patch matrix"""
    x = u.probe_activation(dict(c, id=c["id"]))
    want = torch.from_numpy(u.unfold(x, c["gg"]).astype(np.float32)).cuda()
    a = u.t16(x, dtype).cuda()
    bad = []
    if c["mode"] != 2:
        Kp = u.cdiv(c["M"], 64) * 64
        col = _im2col16(lib, a, c["gg"], c["C"], Kp, dtype)
        if not torch.equal(col[:, :c["M"]].float(), want) or bool((col[:, c["M"]:] != 0).any()):
            bad.append("probe: eoe_im2col differs from the unfold")
    N = c["N"] if c["T"] <= 16 * c["N"] else 136
    for t0 in range(0, c["T"], N):
        w = min(N, c["T"] - t0)
        dy = torch.zeros(c["T"], N, dtype=dtype)
        dy[t0 + torch.arange(w), torch.arange(w)] = 1
        dy = dy.cuda()
        out = torch.full((c["M"], N), NAN, dtype=torch.float32, device="cuda")
        _run_tn(lib, u.tn_args(c, dtype, {"a": a.data_ptr(), "b": dy.data_ptr(), "C": out.data_ptr()}, ws.data_ptr(), ws.numel(), N=N,
                               plain=True))
        if not torch.equal(out[:, :w].t(), want[t0:t0 + w]) or bool((out[:, w:] != 0).any()):
            bad.append(f"probe: rows {t0}..{t0 + w} of the patch matrix differ ({int((out[:, :w].t() != want[t0:t0 + w]).sum())} elements)")
            break
    return bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("which", ["mode1", "mode2", "split"])
def test_gemm_tn_gather_at_its_edges(lib, ncu, tn_ws, which, dtype):
    cases = [c for c in u.tn_table() if (which == "split") == c["split"] and (c["split"] or which == f"mode{c['mode']}")]
    assert cases
    bad = {}
    for c in cases:
        if c["split"]:
            assert u.tn_splits(c, ncu)[0] >= 2 and u.tn_splits(c, ncu)[1] % (c["gg"]["Ho"] * c["gg"]["Wo"]) != 0, c["id"]
        f = _tn_case_failures(lib, c, dtype, tn_ws, ncu) + _tn_probe_failures(lib, c, dtype, tn_ws)
        if f:
            bad[c["id"]] = f
    assert not bad, bad


def test_gemm_tn_split_without_workspace_needs_a_dense_c(lib):
    c = u.tn_case(1, u.geo("3s1_17x16", 4), 8, 64, ws="none", ldc_pad=True, split=True)
    d = _dev(u.tn_memory(c, torch.float16))
    with pytest.raises(lib.EoeError, match="dense C"):
        _run_tn(lib, u.tn_args(c, torch.float16, _addr(d), None, 0))


# ------------------------------------------------------------------------------------------------ conv.hip, each entry point alone
def _flat_out(rows, cols, ld, dtype, start_vals=None):
    """a canary-surrounded output on the device: (flat, start)"""
    if start_vals is not None:
        flat, start = gu.embed(start_vals, ld, "canary")
    else:
        n, start = gu.layout(rows, cols, ld)
        flat = gu.canary(n, dtype)
    return flat.cuda(), start


def _check_out(flat, start, rows, cols, ld, want, what):
    flat = flat.cpu()
    bad = gu.canary_failures(flat, rows, cols, ld, start, what)
    got = gu.view_of(flat, rows, cols, ld, start)
    ne = gu.bits(got) != gu.bits(want)
    if bool(ne.any()):
        i, j = (int(v) for v in ne.nonzero()[0])
        bad.append(f"bits:{what}: {int(ne.sum())} of {ne.numel()} differ, first at ({i}, {j}): {float(got[i, j])} for {float(want[i, j])}")
    return bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
def test_im2col_three_input_kinds_and_padding_columns(lib, dtype):
    bad = {}
    for r in u.im2col_cases():
        g, cin, Kp = r["g"], r["cin"], r["Kp"]
        M = g["n"] * g["Ho"] * g["Wo"]
        if r["kind"] == 1:
            raw = u.ints("im/" + r["id"], (g["n"], cin, g["H"], g["W"]), -6, 6).astype(np.float64)
            mean, std = u.norm_params(cin)
            x = torch.from_numpy(raw.astype(np.float32)).cuda()
            vals = (raw - mean[None, :, None, None]) / std[None, :, None, None] if r["norm"] else raw
            nhwc = vals.transpose(0, 2, 3, 1)
            mt, st = (torch.from_numpy(v.astype(np.float32)).cuda() for v in (mean, std))
            mp, sp = (mt.data_ptr(), st.data_ptr()) if r["norm"] else (None, None)
        else:
            nhwc = u.ints("im/" + r["id"], (g["n"], g["H"], g["W"], cin)).astype(np.float64)
            x = (u.t16(nhwc, dtype) if r["kind"] == 0 else torch.from_numpy(nhwc.astype(np.float32))).cuda()
            mp = sp = None
        # the unfold only moves values: applied to the two halves of a value split exactly, it moves any value
        want = u.rne16(_unfold_float(nhwc, g, Kp), dtype)
        flat, start = _flat_out(M, Kp, Kp, dtype)
        flat[start:start + M * Kp] = NAN
        lib.check(lib.lib.eoe_im2col(x.data_ptr(), r["kind"], mp, sp, flat.data_ptr() + start * 2, g["n"], cin, g["H"], g["W"], g["kh"], g["kw"],
                                     g["s"], g["p"], Kp, _dcode(lib, dtype), _stream()), "eoe_im2col")
        torch.cuda.synchronize()
        f = _check_out(flat, start, M, Kp, Kp, want, "patches")
        if f:
            bad[r["id"]] = f
    assert not bad, bad


def _unfold_float(nhwc, g, Kp):
    """unfold of quarter-integers: scaled to integers, moved, scaled back (exact)"""
    q = np.rint(nhwc * 4).astype(np.int64)
    assert np.array_equal(q / 4.0, nhwc)
    return u.unfold(q, g, Kp=Kp) / 4.0


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
def test_col2im_strides_one_wide_maps_and_accumulate(lib, dtype):
    bad = {}
    for r in u.col2im_cases():
        g, Cc, Kp = r["g"], r["C"], r["Kp"]
        M, P = g["n"] * g["Ho"] * g["Wo"], g["n"] * g["H"] * g["W"]
        dp = u.ints("dp/" + r["id"], (M, Kp)).astype(np.float64)
        want = u.col2im_ref(dp.astype(np.int64), g, Cc)[0].reshape(P, Cc).astype(np.float64)
        dp[:, g["kh"] * g["kw"] * Cc:] = NAN                                    # the Kp tail is never read
        dx0 = u.ints("dx0/" + r["id"], (P, Cc))
        if r["accumulate"]:
            want = want + dx0
            flat, start = _flat_out(P, Cc, Cc, torch.float32, torch.from_numpy(dx0.astype(np.float32)))
        else:
            flat, start = _flat_out(P, Cc, Cc, torch.float32)
            flat[start:start + P * Cc] = NAN
        d16 = torch.from_numpy(dp.astype(np.float32)).to(dtype).cuda()
        lib.check(lib.lib.eoe_col2im(d16.data_ptr(), flat.data_ptr() + start * 4, g["n"], Cc, g["H"], g["W"], g["kh"], g["kw"], g["s"], g["p"],
                                     Kp, _dcode(lib, dtype), r["accumulate"], _stream()), "eoe_col2im")
        torch.cuda.synchronize()
        f = _check_out(flat, start, P, Cc, Cc, torch.from_numpy(want.astype(np.float32)), "dx")
        if f:
            bad[r["id"]] = f
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("count", [1, 33])
def test_conv_pack_weight_multi_writes_exactly_its_layouts(lib, count, dtype):
    """1 job and 33 (a second batch behind PACK_MAX_JOBS = 32, its block_start from 0): every output NaN-filled inside canaries first"""
    jobs = u.pack_jobs(count)
    arr, keep, outs = (lib.ConvPackJob * count)(), [], []
    for i, j in enumerate(jobs):
        taps = j["kh"] * j["kw"]
        w = torch.from_numpy(j["w"].astype(np.float32)).cuda()
        shapes = {"w16": (j["cout"], j["Kp"]), "w16t": (j["Kp"], j["cout"]) if j["t"] else None, "w16d": (j["cin"] * taps, j["cout"]) if j["d"] else None}
        o = {}
        for n, s in shapes.items():
            if s is not None:
                flat, start = _flat_out(s[0], s[1], s[1], dtype)
                flat[start:start + s[0] * s[1]] = NAN
                o[n] = (flat, start, s)
        p = lambda n: o[n][0].data_ptr() + o[n][1] * 2 if n in o else None   # noqa: E731
        arr[i] = lib.ConvPackJob(w.data_ptr(), p("w16"), p("w16t"), p("w16d"), j["cout"], j["cin"], j["cpad"], j["kh"], j["kw"], j["Kp"])
        keep.append(w)
        outs.append(o)
    lib.check(lib.lib.eoe_conv_pack_weight_multi(arr, count, _dcode(lib, dtype), _stream()), "eoe_conv_pack_weight_multi")
    torch.cuda.synchronize()
    bad = {}
    for i, (j, o) in enumerate(zip(jobs, outs)):
        ref = dict(zip(("w16", "w16t", "w16d"), u.pack_ref(j["w"], j["cpad"], j["Kp"])))
        for n, (flat, start, s) in o.items():
            f = _check_out(flat, start, s[0], s[1], s[1], u.t16(ref[n], dtype), n)
            if f:
                bad[f"job{i}:{n}"] = f
    assert not bad, bad


def test_conv_unpack_wgrad_both_layouts_and_pack_round_trip(lib):
    bad = {}
    for i, j in enumerate(u.pack_jobs(7)):
        cout, cin, cpad, kh, kw, Kp = (j[n] for n in ("cout", "cin", "cpad", "kh", "kw", "Kp"))
        w16, w16t, _ = u.pack_ref(j["w"], cpad, Kp)
        dw0 = u.ints(f"dw0/{i}", j["w"].shape)
        for transposed in (0, 1):
            for acc in (0, 1):
                gsrc = w16t[:kh * kw * cpad] if transposed else w16
                g = torch.from_numpy(np.ascontiguousarray(gsrc).astype(np.float32)).cuda()
                flat, start = _flat_out(cout, cin * kh * kw, cin * kh * kw, torch.float32,
                                        torch.from_numpy(dw0.astype(np.float32)).reshape(cout, -1) if acc else None)
                lib.check(lib.lib.eoe_conv_unpack_wgrad(g.data_ptr(), flat.data_ptr() + start * 4, cout, cin, cpad, kh, kw, Kp, transposed, acc,
                                                        _stream()), "eoe_conv_unpack_wgrad")
                torch.cuda.synchronize()
                want = torch.from_numpy((j["w"] + (dw0 if acc else 0)).astype(np.float32)).reshape(cout, -1)
                f = _check_out(flat, start, cout, cin * kh * kw, cin * kh * kw, want, "dw")
                if f:
                    bad[f"job{i}-t{transposed}-acc{acc}"] = f
        # the kernels' own round trip: pack on the device (fp16 holds the integers), unpack its w16 and its w16t
        w = torch.from_numpy(j["w"].astype(np.float32)).cuda()
        p16, p16t = torch.empty(cout, Kp, dtype=torch.float16, device="cuda"), torch.empty(Kp, cout, dtype=torch.float16, device="cuda")
        lib.check(lib.lib.eoe_conv_pack_weight(w.data_ptr(), p16.data_ptr(), p16t.data_ptr(), None, cout, cin, cpad, kh, kw, Kp, lib.EOE_F16,
                                               _stream()), "eoe_conv_pack_weight")
        for transposed, src in ((0, p16.float()), (1, p16t.float())):
            back = torch.full_like(w, NAN)
            lib.check(lib.lib.eoe_conv_unpack_wgrad(src.data_ptr(), back.data_ptr(), cout, cin, cpad, kh, kw, Kp, transposed, 0, _stream()),
                      "eoe_conv_unpack_wgrad")
            torch.cuda.synchronize()
            if not torch.equal(back, w):
                bad[f"job{i}-roundtrip-t{transposed}"] = "pack -> unpack does not return the weights"
    assert not bad, bad


STEM_IMAGES = ((2, 9, 7, 1, 4, (2, 3)), (3, 5, 12, 3, 8, (0, 0)), (2, 1, 5, 0, 4, (4, 1)), (2, 6, 1, 2, 8, (1, 5)))     # n, H, W, pad, cpad, slack


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
def test_stem_pack_image_border_and_channel_padding(lib, dtype):
    bad = {}
    for n, H, W, pad, cpad, slack in STEM_IMAGES:
        for norm in (False, True):
            Hp, Wp = H + pad + slack[0], W + pad + slack[1]
            raw = u.ints(f"stemimg/{n}x{H}x{W}", (n, 3, H, W), -6, 6).astype(np.float64)
            mean, std = u.norm_params(3)
            vals = (raw - mean[None, :, None, None]) / std[None, :, None, None] if norm else raw
            want = u.rne16(u.stem_pack_image_ref(vals, dict(Hp=Hp, Wp=Wp, p=pad), cpad), dtype).reshape(n * Hp * Wp, cpad)
            x = torch.from_numpy(raw.astype(np.float32)).cuda()
            mt, st = (torch.from_numpy(v.astype(np.float32)).cuda() for v in (mean, std))
            flat, start = _flat_out(n * Hp * Wp, cpad, cpad, dtype)
            flat[start:start + n * Hp * Wp * cpad] = NAN
            lib.check(lib.lib.eoe_stem_pack_image(x.data_ptr(), mt.data_ptr() if norm else None, st.data_ptr() if norm else None,
                                                  flat.data_ptr() + start * 2, n, H, W, Hp, Wp, pad, cpad, _dcode(lib, dtype), _stream()),
                      "eoe_stem_pack_image")
            torch.cuda.synchronize()
            f = _check_out(flat, start, n * Hp * Wp, cpad, cpad, want, "image")
            if f:
                bad[f"{n}x{H}x{W}-pad{pad}-cpad{cpad}-norm{norm}"] = f
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
def test_stem_pack_weight_and_unpack_wgrad(lib, dtype):
    bad = {}
    for cout, kh, kw in ((8, 3, 7), (72, 7, 3), (40, 8, 8), (64, 2, 5)):
        w = u.ints(f"stemw/{cout}x{kh}x{kw}", (cout, 3, kh, kw))
        K = u.cdiv(kh, 2) * 64
        ref = u.stem_pack_weight_ref(w)
        wd = torch.from_numpy(w.astype(np.float32)).cuda()
        flat, start = _flat_out(cout, K, K, dtype)
        flat[start:start + cout * K] = NAN
        lib.check(lib.lib.eoe_stem_pack_weight(wd.data_ptr(), flat.data_ptr() + start * 2, cout, kh, kw, _dcode(lib, dtype), _stream()),
                  "eoe_stem_pack_weight")
        torch.cuda.synchronize()
        f = _check_out(flat, start, cout, K, K, u.t16(ref, dtype), "w16")
        # the inverse: gT [K, cout] (here the packed weights themselves, transposed; junk where the pack holds zeros) -> [cout, 3, kh, kw]
        junk = np.where(u.stem_pack_weight_ref(np.ones_like(w)) == 1, ref, 7)
        gT = torch.from_numpy(np.ascontiguousarray(junk.T).astype(np.float32)).cuda()
        flat2, start2 = _flat_out(cout, 3 * kh * kw, 3 * kh * kw, torch.float32)
        lib.check(lib.lib.eoe_stem_unpack_wgrad(gT.data_ptr(), flat2.data_ptr() + start2 * 4, cout, kh, kw, _stream()), "eoe_stem_unpack_wgrad")
        torch.cuda.synchronize()
        f += _check_out(flat2, start2, cout, 3 * kh * kw, 3 * kh * kw, torch.from_numpy(w.astype(np.float32)).reshape(cout, -1), "dw")
        if f:
            bad[f"{cout}x{kh}x{kw}"] = f
    assert not bad, bad


@pytest.mark.parametrize("dtype", u.DTYPES, ids=DT_IDS)
def test_stem_round_trip_equals_the_unfold_of_the_unpacked_layer(lib, dtype):
    """eoe_stem_pack_image + eoe_stem_pack_weight + eoe_gemm_nt mode 2 = the 3-channel convolution from its definition"""
    bad = {}
    for c in u.nt_table()["nt64_g2"]:
        g, N = c["g"], c["N"]
        raw, w = u.ints(f"img/{g['name']}/{g['n']}", (g["n"], 3, g["H"], g["W"])), u.stem_weight(c)
        x, wd = torch.from_numpy(raw.astype(np.float32)).cuda(), torch.from_numpy(w.astype(np.float32)).cuda()
        img = torch.full((g["n"], g["Hp"], g["Wp"], 4), NAN, dtype=dtype, device="cuda")
        w16 = torch.full((N, c["K"]), NAN, dtype=dtype, device="cuda")
        lib.check(lib.lib.eoe_stem_pack_image(x.data_ptr(), None, None, img.data_ptr(), g["n"], g["H"], g["W"], g["Hp"], g["Wp"], g["p"], 4,
                                              _dcode(lib, dtype), _stream()), "eoe_stem_pack_image")
        lib.check(lib.lib.eoe_stem_pack_weight(wd.data_ptr(), w16.data_ptr(), N, g["kh"], g["kw"], _dcode(lib, dtype), _stream()),
                  "eoe_stem_pack_weight")
        out = torch.full((c["M"], N), NAN, dtype=torch.float32, device="cuda")
        args = u.nt_args(dict(c, ldb=c["K"]), dtype, {"a": img.data_ptr(), "b": w16.data_ptr(), "C": out.data_ptr()}, out_f32=True, plain=True)
        f = _run_nt(lib, c, args)
        plain = dict(name=g["name"], n=g["n"], kh=g["kh"], kw=g["kw"], s=g["s"], p=g["p"], H=g["H"], W=g["W"], Ho=g["Ho"], Wo=g["Wo"])
        want = u.unfold(raw.transpose(0, 2, 3, 1), plain) @ w.transpose(0, 2, 3, 1).reshape(N, -1).T
        if not torch.equal(out.cpu(), torch.from_numpy(want.astype(np.float32))):
            f.append("the packed first layer differs from the convolution of the unpacked one")
        if f:
            bad[c["id"]] = f
    assert not bad, bad
