"""Keeps the table of tests/test_gpu_grid_stride.py honest (no GPU needed): every __global__ kernel of gridpp_amd/csrc outside the OI and
EnSI units whose body holds a loop that steps by gridDim.x (times a constant, directly or through a `stride` / `step` variable) is named in
that table or exempted below with a reason, and no .hip file sizes the grid of such a kernel with a bare std::min where grid_capped -- the
one place GPP_GRID_CAP acts -- would do.  A new capped kernel cannot arrive without a second-trip test."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gridpp_amd", "csrc")
OWN_STRESS_TESTS = ("oi", "ensi")            # units whose tile loops have stress tests of their own (file name prefixes)

# kernels with a loop over gridDim.x that need no case in the table: name -> why
EXEMPT = {
}


def sources(ext):
    out = []
    for p in sorted(glob.glob(os.path.join(CSRC, "*" + ext))):
        name = os.path.basename(p)
        if not any(name == u + ext or name.startswith(u + "_") or name.startswith(u + ".") for u in OWN_STRESS_TESTS):
            out.append(p)
    return out


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)
    return re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), text)


def matching(text, start, open_ch, close_ch):
    """index just behind the bracket that closes the one at text[start]"""
    depth = 0
    for i in range(start, len(text)):
        if text[i] == open_ch:
            depth += 1
        elif text[i] == close_ch:
            depth -= 1
            if depth == 0:
                return i + 1
    raise ValueError("unbalanced %s at %d" % (open_ch, start))


def kernels(text):
    """(name, body) of every __global__ function of a source text without comments"""
    for m in re.finditer(r"__global__", text):
        paren = text.index("(", m.end())
        while text[m.end():paren].strip().endswith("__launch_bounds__"):        # skip __launch_bounds__(...)
            paren = text.index("(", matching(text, paren, "(", ")"))
        name = re.findall(r"(\w+)\s*$", text[m.end():paren])[0]
        brace = text.index("{", matching(text, paren, "(", ")"))
        yield name, text[brace:matching(text, brace, "{", "}")]


GRID_X = r"(?:\([\w\s]+\)\s*)?gridDim\.x(?:\s*\*\s*[\w().\s*]+?)?"


def strides_over_grid(body):
    if re.search(r"\+=\s*" + GRID_X + r"\s*\)", body):
        return True
    names = re.findall(r"\b(\w+)\s*=\s*" + GRID_X + r"\s*[;,]", body)
    return any(re.search(r"\+=\s*%s\s*\)" % re.escape(n), body) for n in names)


def striding_kernels():
    found = {}
    for p in sources(".hip") + sources(".h"):
        with open(p) as f:
            for name, body in kernels(strip_comments(f.read())):
                if strides_over_grid(body):
                    found[name] = os.path.basename(p)
    return found


def table_kernels():
    with open(os.path.join(ROOT, "tests", "test_gpu_grid_stride.py")) as f:
        doc = f.read().split('"""')[1]
    rows = [l for l in doc.splitlines() if l.startswith("k_")]
    return {k for l in rows for k in re.findall(r"\bk_\w+", l.split("  ")[0])}


def split_args(text):
    """the top-level arguments of a call's argument text"""
    out, depth, cur = [], 0, ""
    for ch in text:
        if ch in "(<[{":
            depth += 1
        elif ch in ")>]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    return out + [cur.strip()]


def hand_clamped_launches(text, striding):
    """launches of a striding kernel whose grid is a std::min (written in the call, or the variable the call names)"""
    bad = []
    for m in re.finditer(r"\blaunch(_on)?\s*\(", text):
        end = matching(text, m.end() - 1, "(", ")")
        args = split_args(text[m.end():end - 1])
        if m.group(1):
            args = args[1:]                                            # launch_on(stream, kernel, grid, ...)
        if len(args) < 2:
            continue
        kernel = re.sub(r"<.*", "", args[0]).strip()
        if kernel not in striding:
            continue
        grid = args[1]
        ident = re.fullmatch(r"(?:\(\s*[\w\s]+\)\s*)?(\w+)", grid)     # a variable, perhaps behind a cast: its last definition above the call
        if ident:
            defs = re.findall(r"\b%s\s*=\s*([^;]*);" % re.escape(ident.group(1)), text[:m.start()])
            grid = defs[-1] if defs else grid
        if re.search(r"\b(std::)?min\s*[<(]", grid) and "grid_capped" not in grid:
            bad.append((kernel, " ".join(grid.split())))
    return bad


def test_the_scanner_sees_the_loop_forms_of_the_library():
    assert strides_over_grid("{ for(long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { } }")
    assert strides_over_grid("{ for(size_t c0 = (size_t)blockIdx.x * 256; c0 < C; c0 += (size_t)gridDim.x * 256) { } }")
    assert strides_over_grid("{ const long long stride = (long long)gridDim.x * blockDim.x; for(long long i = 0; i < n; i += stride) { } }")
    assert strides_over_grid("{ const size_t total = (size_t)Y * runs, stride = (size_t)gridDim.x * blockDim.x; for(size_t i = 0; i < total; i += stride) x(); }")
    assert not strides_over_grid("{ const long per = ((long)len + gridDim.x - 1) / gridDim.x; for(long i = i0; i < i1; i += 256) { } }")
    assert not strides_over_grid("{ const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x; }")


def test_every_striding_kernel_is_in_the_table_or_exempt():
    found, table = striding_kernels(), table_kernels()
    for name in ("k_rank_tile", "k_rows_tile", "k_rows_block", "k_rowsq_tile", "k_window_scan", "k_window_gather", "k_structure_corr_many", "k_crps_long",
                 "k_fss_cols", "k_score_counts", "k_pointwise", "k_gamma_inv", "k_mo_keys", "k_member_pass", "k_qf_count", "k_curve_shared"):
        assert name in found, name                                      # the scanner finds what the issue lists
    assert not [k for k in found if k.startswith("k_split_")]           # a 2-D partition: the grid's x size IS the split of a row, no loop over it
    missing = sorted(k for k in found if k not in table and k not in EXEMPT)
    assert not missing, "kernels with a loop over gridDim.x and no case in tests/test_gpu_grid_stride.py: %s" % [(k, found[k]) for k in missing]
    stale = sorted(k for k in EXEMPT if k not in found or k in table)
    assert not stale, stale
    assert all(len(why) > 20 for why in EXEMPT.values())
    gone = sorted(k for k in table if k not in found)
    assert not gone, "the table names kernels that no longer stride over the grid: %s" % gone


def test_no_launch_grid_is_clamped_by_hand():
    striding = striding_kernels()
    bad = []
    for p in sources(".hip"):
        with open(p) as f:
            bad += [(os.path.basename(p),) + b for b in hand_clamped_launches(strip_comments(f.read()), striding)]
    assert not bad, "grids sized with std::min where grid_capped would do (GPP_GRID_CAP does not reach them): %s" % bad


def test_the_clamp_check_fails_on_the_forms_it_replaced():
    """the four launch sites as they stood before grid_capped took them over, and two forms that must pass"""
    striding = {"k_rows_tile": "", "k_rows_block": "", "k_rowsq_tile": "", "k_structure_corr_many": "", "k_split_count": ""}
    before = [
        "const long grid = std::min<long>((rows + 63) / 64, 256 * waves_per_cu);\n launch(k_rows_tile, (unsigned)grid, 64, lds, d_in, rows);",
        "launch(k_rows_block, (unsigned)std::min<long>(rows, 256 * 8), 256, 0, d_in, rows, len, d_q, q_per_row, d_out);",
        "const long grid = std::min<long>((rows + 63) / 64, 1L << 20);\n launch(k_rowsq_tile, (unsigned)grid, 64, lds, d_in);",
        "const long long blocks = std::min((n + CORR_BLOCK - 1) / CORR_BLOCK, CORR_MAX_BLOCKS);\n launch(k_structure_corr_many, (unsigned)blocks, CORR_BLOCK, 0, d);",
    ]
    for text in before:
        assert len(hand_clamped_launches(text, striding)) == 1, text
    after = [
        "launch(k_rows_block, grid_capped(rows, 256 * 8), 256, 0, d_in, rows, len, std::min(a, b));",
        "const unsigned tiles = grid_capped(std::max<size_t>(blocks_of(Y, 64), 1), CAP);\n launch(k_rows_tile, tiles, 64, 0, in);",
        "launch(k_not_striding, (unsigned)std::min<long>(rows, 8), 256, 0, d_in);",
    ]
    for text in after:
        assert hand_clamped_launches(text, striding) == [], text
