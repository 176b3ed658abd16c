"""The restated dispatch rule of the row-register aggregator kernels (agg_rows_common.py), pinned without a GPU: the layout cells
as csrc/sgl_core.cpp documents them, that the rule only ever names compiled instances, that every compiled instance is
reachable from some (d, H, tuning) -- so the case list of test_gpu_agg_variants.py can reach all of them -- that the library's own
rule (sgl::row_instance, host code built with g++) equals the restatement, and the parser of the kernel names a profiler reports."""
import itertools
import os
import shutil
import subprocess

import pytest

from agg_rows_common import (FAMILIES, KERNELS, N_ROWS, TUNING_DEFAULTS, TUNING_VALUES, WIDTH_8X5, case_list, compiled_variants,
                             expected_kernel, hmax_of, parse_agg_kernel_name, pick_lpr, pick_row_layout)
from spmm_order_common import parse_kernel_name

HOPS = range(1, 17)
TUNINGS = [dict(row_lpr32x2=a, row_narrow_groups=b) for a, b in itertools.product(TUNING_VALUES["row_lpr32x2"],
                                                                                   TUNING_VALUES["row_narrow_groups"])]


def test_lanes_per_row():
    for d in range(1, 1200):
        lanes = (d + 3) // 4
        assert pick_lpr(d, 4) == (8 if lanes <= 8 else 16 if lanes <= 16 else 32 if lanes <= 32 else 64), d
        assert pick_lpr(d, 1) == (8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64), d


def test_layout_cells_with_default_keys():
    for d in range(1, 513):
        for H in HOPS:
            want = ((8, 1) if d <= 32 else (16, 1) if d <= 64 else (32, 1) if d <= 128 else
                    ((16, 3) if H <= 12 else (32, 2)) if d <= 192 else (32, 2) if d <= 256 else (64, 2))
            assert pick_row_layout(d, H) == want, (d, H)
            assert pick_row_layout(d, H, tuning=TUNING_DEFAULTS) == want, (d, H)
            # 8 x 5: only where allowed, for rows of 129..160 floats and at most 6 hops
            assert pick_row_layout(d, H, allow_8x5=True) == ((8, 5) if 129 <= d <= 160 and H <= 6 else want), (d, H)


def test_64x1_needs_row_lpr32x2_off():
    for d in range(1, 513):
        for H in HOPS:
            for allow in (False, True):
                for mode in TUNING_VALUES["row_narrow_groups"]:
                    assert pick_row_layout(d, H, allow, dict(row_lpr32x2=1, row_narrow_groups=mode)) != (64, 1), (d, H, allow, mode)
                off = pick_row_layout(d, H, allow, dict(row_lpr32x2=0, row_narrow_groups=0))
                assert (off == (64, 1)) == (129 <= d <= 256), (d, H, allow)
                # with both keys off the rule is pick_lpr alone plus a second chunk
                assert off == (pick_lpr(d, 4), 2 if d > 256 else 1), (d, H)


def test_narrow_group_modes():
    for d in range(1, 513):
        for H in HOPS:
            for lpr32 in (0, 1):
                wide = pick_row_layout(d, H, True, dict(row_lpr32x2=lpr32, row_narrow_groups=0))
                in16, in8 = 129 <= d <= 192 and H <= 12, 129 <= d <= 160 and H <= 6
                assert pick_row_layout(d, H, True, dict(row_lpr32x2=lpr32, row_narrow_groups=2)) == ((16, 3) if in16 else wide)
                assert pick_row_layout(d, H, True, dict(row_lpr32x2=lpr32, row_narrow_groups=3)) == ((8, 5) if in8 else wide)
                assert pick_row_layout(d, H, False, dict(row_lpr32x2=lpr32, row_narrow_groups=3)) == wide
                assert pick_row_layout(d, H, True, dict(row_lpr32x2=lpr32, row_narrow_groups=1)) == ((8, 5) if in8 else (16, 3) if in16 else wide)


def test_hop_capacity_tables():
    for lay in ((8, 1), (64, 2), (32, 2)):
        assert [hmax_of(lay, h) for h in range(1, 17)] == [2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, 14, 14, 16, 16]
        assert hmax_of(lay, 17) is None and hmax_of(lay, 0) is None
    assert [hmax_of((16, 3), h) for h in range(1, 14)] == [2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 12, 12, None]
    assert [hmax_of((8, 5), h) for h in range(1, 8)] == [2, 2, 4, 4, 6, 6, None]


def test_variant_counts():
    assert {f: len(compiled_variants(f)) for f in FAMILIES} == {"rowdot_reg": 108, "nafs": 54, "gate": 54, "recursive": 54,
                                                                 "rowdot2": 57, "prefix": 7}


@pytest.mark.parametrize("family", FAMILIES)
def test_rule_names_exactly_the_compiled_instances(family):
    """expected_kernel over every width, hop count and key value is a subset of the compiled set, and reaches all of it"""
    seen = set()
    for tuning in TUNINGS:
        for d in range(1, 513):
            for H in HOPS:
                for gu in ((False, True) if family == "rowdot_reg" else (False,)):
                    fam, var = expected_kernel(family, d, H, tuning, g_unaligned=gu)
                    assert fam == family
                    seen.add(var)
    compiled = compiled_variants(family)
    assert seen == compiled, ("named, not compiled", sorted(seen - compiled), "compiled, never named", sorted(compiled - seen))


@pytest.mark.parametrize("family", FAMILIES)
def test_gpu_case_list_reaches_every_compiled_instance(family):
    """the cases test_gpu_agg_variants.py launches: every one has a fused kernel, together they name the whole compiled set, every
    layout has a one-row case, and every case has a partial last block"""
    cases = case_list(family)
    assert len(cases) == len({(n, d, h, tuple(sorted(t.items()))) for n, d, h, t in cases})
    seen, one_row = set(), set()
    for n, d, h, tuning in cases:
        for gu in ((False, True) if family == "rowdot_reg" else (False,)):
            fam, var = expected_kernel(family, d, h, tuning, g_unaligned=gu)
            seen.add(var)
            if n == 1:
                one_row.add(var[:2])
            else:
                assert n == N_ROWS and n % (256 // var[0]) != 0 and n > 2 * (256 // 8)
    assert seen == compiled_variants(family), sorted(compiled_variants(family) - seen)
    assert one_row == {v[:2] for v in compiled_variants(family)}
    if family == "rowdot2":                                # 8 x 5 gives way to 16 x 3 at 7 hops
        assert expected_kernel(family, WIDTH_8X5, 6)[1] == (8, 5, 6) and expected_kernel(family, WIDTH_8X5, 7)[1] == (16, 3, 8)
    if family != "prefix":                                 # 16 x 3 gives way to 32 x 2 at 13 hops
        assert expected_kernel(family, 147, 12)[1][:3] == (16, 3, 12) and expected_kernel(family, 147, 13)[1][:3] == (32, 2, 14)


@pytest.mark.parametrize("family", FAMILIES)
def test_general_path_boundaries(family):
    assert expected_kernel(family, 513, 4) is None
    assert expected_kernel(family, 512, 4, aligned=False) is None
    assert expected_kernel(family, 512, 16) is not None
    if family == "prefix":
        assert expected_kernel(family, 147, 40) == ("prefix", (16, 3))      # any hop count, the layout of one hop
    else:
        assert expected_kernel(family, 100, 17) is None


def test_library_row_rule_equals_the_restatement(tmp_path):
    """sgl::row_instance / sgl::out_cols (csrc/sgl_core.cpp: pure host code), built with g++ into tests/native/agg_rows_table.cpp
    and asked once for every d in 1 .. 520, every hop count in 1 .. 17, 8 x 5 allowed or not, and every value of the three tuning
    keys one key at a time: (lpr, ch) is pick_row_layout's, hmax is hmax_of's with 0 exactly where that is None, and every answer
    with hmax > 0 is a compiled instance of the family that may (rowdot2) or may not (nafs) use 8 x 5.  out_cols, for 0 / 3 / 13
    declared pad columns and the room of the layout: the d data columns, plus the pad when row_whole_lines is set, as far as the
    layout's lanes reach, and then only as whole 16-byte vectors."""
    from conftest import ROOT
    gxx = shutil.which("g++")
    if gxx is None or not os.path.exists("/opt/rocm/include/hip/hip_runtime.h"):
        pytest.skip("needs g++ and the HIP headers")
    exe = str(tmp_path / "agg_rows_table")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        os.path.join(ROOT, "tests", "native", "agg_rows_table.cpp"), os.path.join(ROOT, "sgl_amd", "csrc", "sgl_core.cpp"),
                        "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-pthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    keys = ("row_lpr32x2", "row_narrow_groups", "row_whole_lines")
    tunings = [{}] + [{k: v} for k in keys for v in TUNING_VALUES[k]]
    cases = [(d, H, allow, pad, t) for t in tunings for allow in (0, 1) for d in range(1, 521) for H in range(1, 18) for pad in (0, 3, 13)]
    queries = [f"{d} {H} {allow} {pad} " + " ".join(str(t.get(k, TUNING_DEFAULTS[k])) for k in keys) for d, H, allow, pad, t in cases]
    r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(cases) == 9 * 2 * 520 * 17 * 3
    compiled = {0: compiled_variants("nafs"), 1: compiled_variants("rowdot2")}
    seen, none_seen = {0: set(), 1: set()}, 0
    for (d, H, allow, pad, t), (lpr, ch, hmax, cols) in zip(cases, got):
        lay = pick_row_layout(d, H, bool(allow), t)
        want = hmax_of(lay, H)
        assert (lpr, ch) == lay and hmax == (0 if want is None else want), ((d, H, allow, t), (lpr, ch, hmax), lay, want)
        none_seen += want is None
        if hmax > 0:
            assert (lpr, ch, hmax) in compiled[allow], ((d, H, allow, t), (lpr, ch, hmax))
            seen[allow].add((lpr, ch, hmax))
        room, dw = lpr * ch * 4, d + pad if t.get("row_whole_lines", 1) else d
        if dw > room:
            dw = room // 4 * 4 if room > d else d
        if dw > d and dw % 4:
            dw = d
        assert cols == dw, ((d, H, allow, pad, t), cols, dw)
    assert seen == compiled                                   # the queries reach every instance of both tables
    assert none_seen == 9 * 2 * 520 * 3                       # 17 hops: no layout has an instance, whatever the keys say


def test_kernel_name_parser():
    ns = "void (anonymous namespace)::"
    assert parse_agg_kernel_name(ns + "nafs_fused_kernel<32, 2, 6>(Hops, int, float*, long, float*, long, long, int, int)") == ("nafs", (32, 2, 6))
    assert parse_agg_kernel_name(ns + "gate_fused_kernel<(int)16, (int)3, (int)12>(Hops)") == ("gate", (16, 3, 12))
    assert parse_agg_kernel_name(ns + "recursive_fused_kernel<8, 1, 16>(Hops)") == ("recursive", (8, 1, 16))
    assert parse_agg_kernel_name(ns + "hop_rowdot2_reg_kernel<8, 5, 6>(Hops)") == ("rowdot2", (8, 5, 6))
    assert parse_agg_kernel_name(ns + "nafs_prefix_kernel<64, 1>(Hops)") == ("prefix", (64, 1))
    for spelled, gu in (("(bool)1", 1), ("true", 1), ("(bool)0", 0), ("false", 0)):
        assert parse_agg_kernel_name(ns + f"hop_rowdot_reg_kernel<64, 2, 14, {spelled}>(Hops, int)") == ("rowdot_reg", (64, 2, 14, gu))
    assert parse_agg_kernel_name("_ZN12_GLOBAL__N_121hop_rowdot_reg_kernelILi16ELi3ELi6ELb1EEEv4HopsiPKflPflli") == ("rowdot_reg", (16, 3, 6, 1))
    assert parse_agg_kernel_name("_ZN12_GLOBAL__N_121hop_rowdot_reg_kernelILi8ELi1ELi2ELb0EEEv4HopsiPKflPflli") == ("rowdot_reg", (8, 1, 2, 0))
    assert parse_agg_kernel_name("_ZN12_GLOBAL__N_122hop_rowdot2_reg_kernelILi8ELi5ELi4EEEv4Hops") == ("rowdot2", (8, 5, 4))
    assert parse_agg_kernel_name("_ZN12_GLOBAL__N_117nafs_fused_kernelILi64ELi1ELi16EEEv4Hops") == ("nafs", (64, 1, 16))
    assert parse_agg_kernel_name("_ZN12_GLOBAL__N_118nafs_prefix_kernelILi16ELi3EEEv4Hops") == ("prefix", (16, 3))
    # the general-path kernels and everything else are not of the six families
    for other in (ns + "hop_rowdot_kernel<64, 4>(Hops)", ns + "nafs_weight_kernel<8, 4>(Hops)", ns + "hop_wsum2d_kernel<4, true>(Hops)",
                  ns + "recursive_scalar_bwd_kernel<8>(int)", "spmm_kernel<4, 64, 1, 16, false, false>(A)", "Memcpy DtoH"):
        assert parse_agg_kernel_name(other) is None, other
    # a family kernel without its template arguments cannot be identified: an error, not a pass
    for broken in (ns + "nafs_fused_kernel", ns + "gate_fused_kernel<32, 2>(Hops)", ns + "hop_rowdot_reg_kernel<8, 1, 2>(Hops)"):
        with pytest.raises(ValueError):
            parse_agg_kernel_name(broken)
    assert set(KERNELS) == set(FAMILIES)
    # the argument parser is shared with the SpMM name parser, which still reads its names
    assert parse_kernel_name("void spmm_kernel<4, 64, 1, 16, (bool)1, false>(A)") == ("f32", (4, 64, 1, 16, 1))
    assert parse_kernel_name("_ZN3sgl16spmm_bf16_kernelILi8ELi64ELi1ELi16EEEvPKv") == ("bf16", (8, 64, 1, 16))
