"""Case tables of the narrow-width tests (tests/test_gpu_rowops_narrow.py, tests/test_gpu_vit_narrow.py, tests/test_cpu_vit_narrow.py):
LayerNorm forward / backward and embed + ln_pre at widths that are multiples of 64 but not of 256, where the kernels of
csrc/elementwise.hip predicate the last 256-column group of a row (16, 32 or 48 active lanes), and the tower geometries built on them.

Inputs, fp64 references and every tolerance are those of tests/rowops_util.py (its ln_case / embed_case / ln_specs / embed_specs at the
widths below); nothing is measured anew.  tests/test_cpu_vit_narrow.py checks that the fp32-CPU evaluation of these cases stays inside
REF_ERR32["ln/mean"] / ["ln/rstd"], the two measured constants the specs use."""
import rowops_util as ru

# 64: the tail group alone, 16 lanes; 128: 32 lanes; 192: 48 lanes (ViT-Ti); 320: one full group + 16 lanes; 384: + 32 (ViT-S);
# 960: three full groups + 48 lanes (NV = 4); 256: no tail, the control
LN_WIDTHS = (64, 128, 192, 320, 384, 960, 256)
TAIL_WIDTHS = tuple(D for D in LN_WIDTHS if D % 256)
# 1: one wave; 5: a partial forward workgroup (4 waves); 9: a partial backward workgroup (8 waves); 4100: more than EOE_LN_PARTIALS * 8
# rows, so some waves of the backward take a second row
LN_ROWS = (1, 5, 9, 4100)
LN_INST_ROWS = 9                          # the instantiation x output-selection sweep
LN_STRIDED_ROWS, LN_MARGIN = 5, 64        # ldx = ld_out = D + LN_MARGIN: the 64 columns a tail group's idle lanes would touch
EMBED_CASES = ((64, 1, 2), (192, 3, 17), (320, 2, 5), (384, 2, 82))          # (D, n, L)
GUARD = 256                               # elements of NaN behind the last row of every output

# towers: (input_resolution, patch, width, layers, output_dim)
TI_SHORT = dict(input_resolution=64, patch_size=16, width=192, layers=2, output_dim=64)        # 17 tokens, 3 heads: short attention
S_LONG = dict(input_resolution=144, patch_size=16, width=384, layers=2, output_dim=64)        # 82 tokens, 6 heads: long attention
ONE_HEAD = dict(input_resolution=32, patch_size=16, width=64, layers=1, output_dim=32)        # 5 tokens, rows of the tail group alone
W320 = dict(input_resolution=32, patch_size=16, width=320, layers=1, output_dim=32)           # 5 tokens, 5 heads
TOWERS = {"ti_short": TI_SHORT, "s_long": S_LONG, "one_head": ONE_HEAD, "w320": W320}
G28_GEOMETRY = (64, 16, 192, 2, 3, 64)

# The fp32-CPU evaluation's row-statistic errors over the cases below, by the procedure of rowops_util.measure() (`python
# tests/vit_narrow_util.py`).  Both lie a little above rowops_util.REF_ERR32 (4.8e-08 / 1.7e-07, measured at its own tables: rows of 64 ..
# 192 elements with 4100 of them draw a worse worst case), so they get keys of their own here.  They are RECORDED, not used: the GPU tests
# keep rowops_util's bounds (bound_factor("ln/mean") = 5.6 ulp, bound_factor("ln/rstd") = 9.7 ulp of the scale), inside which the fp32-CPU
# evaluation of every narrow case still lies (tests/test_cpu_vit_narrow.py).
NARROW_REF_ERR32 = {
    "ln/mean": 5.9e-08,                           # measured 5.863e-08 (0.49 ulp)
    "ln/rstd": 1.8e-07,                           # measured 1.734e-07 (1.45 ulp)
}


def ln_narrow_case(rows, D, dy_dtype=None, with_res=True):
    return ru.ln_case(f"narrow{rows}x{D}", rows, D, dy_dtype, with_res)


def ln_narrow_strided_case(D, dy_dtype, with_res=True):
    return ru.ln_case(f"narrow_strided{D}", LN_STRIDED_ROWS, D, dy_dtype, with_res)


def ln_narrow_cases_all():
    """(what, case, specs) of every LayerNorm case of the narrow tables, for the CPU check"""
    out = []
    for D in LN_WIDTHS:
        for rows in LN_ROWS:
            for dt in ru.DTYPES:
                c = ln_narrow_case(rows, D, dt)
                out.append((f"ln narrow {rows}x{D} {dt}", c, ru.ln_specs("plain", rows, D, c["ref"], dt)))
        for dt in (None,) + ru.DTYPES:
            for with_res in (True, False):
                c = ln_narrow_case(LN_INST_ROWS, D, dt, with_res)
                out.append((f"ln narrow inst {D} {dt} res={with_res}", c, ru.ln_specs("plain", LN_INST_ROWS, D, c["ref"], dt)))
        for dt in ru.DTYPES:
            for with_res in (True, False):
                c = ln_narrow_strided_case(D, dt, with_res)
                out.append((f"ln narrow strided {D} {dt} res={with_res}", c, ru.ln_specs("plain", LN_STRIDED_ROWS, D, c["ref"], dt)))
    return out


def measure_narrow() -> dict:
    """largest scaled error of the fp32-CPU evaluation over the narrow cases, by the procedure of rowops_util.measure()"""
    table = {}
    for _, c, specs in ln_narrow_cases_all():
        ru.measure_into(table, c["got32"], c["ref"], specs)
    for D, n, L in EMBED_CASES:
        c = ru.embed_case(D, n, L)
        ru.measure_into(table, c["got32"], c["ref"], ru.embed_specs(c))
    return table


if __name__ == "__main__":
    for k, v in sorted(measure_narrow().items()):
        print(f'    "{k}": {v:.3e},    # {v / ru.ULP32:.2f} ulp; REF_ERR32 {ru.REF_ERR32[k]:.3e}')
