"""CPU: the staged reference of the heat-map -> boxes kernels (tests/det_post_ref.py) before anything on a device is held to it.

  * its final boxes and confidences, computed from its own stages, equal heatmap.detect_boxes on every page (exactly: the same
    functions finish them) and the native harness (tests/native/det_post_host.cpp = det_post_core.h, the code the kernels run) at
    test_det_post_cpu.py's bar;
  * its thresholds equal get_dynamic_thresholds of the installed numpy bit for bit (a condition on the pages: numpy's float32 pairwise
    mean may differ from the exact mean in the last bit; generated pages are redrawn until it does not, and none may be dropped);
  * every mutant changes a stage of a case that lists it, and every mutant is listed;
  * the pages reach what they were drawn for (component counts, geometry classes, hull size, ties, scan blocks);
  * surya_det_boxes_workspace_layout (host code) agrees with surya_det_boxes_workspace_bytes."""
import ctypes as C

import numpy as np
import pytest

import det_post_ref as R
from surya_amd.detection import heatmap as hm
from test_det_post_cpu import native, run_native  # noqa: F401  (the fixture that builds the harness)

PAGE_NAMES = ["wrap0", "wrap1", "wrap2", "segments_s", "segments_a", "segments_r", "spiral_s", "spiral_r", "comb_top_s", "comb_bottom_s",
              "comb_bottom_r", "nested_s", "serpentine_s", "checker_s", "diagonal_s", "filters_a", "dark_s", "equal_s", "plateau_a", "zero_one_s",
              "low10_s", "mid11_s", "edges_s", "frame_s", "many_a", "squares_a", "big_a", "big_b"]
CASE_NAMES = ["wrap", "topology_a", "topology_b", "topology_c", "segments_a", "overflow", "thresholds_a", "thresholds_b", "plateau", "rows_260",
              "big_a", "big_b"]


def _full(name):
    return R.ref_page(R.page(name), 1 << 20)


def test_no_case_dropped():
    assert sorted(R.PAGES) == sorted(PAGE_NAMES)
    assert [c.name for c in R.CASES] == CASE_NAMES
    used = {n for c in R.CASES for n in c.pages + c.second}
    assert used == set(PAGE_NAMES), set(PAGE_NAMES) ^ used
    for c in R.CASES:
        assert len({R.page(n).shape for n in c.pages + c.second}) == 1, c.name      # one call, one page size
        assert R.page(c.pages[0]).shape[1] % 4 == 0


@pytest.mark.parametrize("name", PAGE_NAMES)
def test_staged_reference_equals_host_and_native(native, name):  # noqa: F811
    heat = R.page(name)
    r = _full(name)
    tt, lt = hm.get_dynamic_thresholds(heat, R.TEXT, R.LOW)
    assert tt.dtype == np.float32 and lt.dtype == np.float32
    assert R.bits(tt) == R.bits(r["text_thr"]) and R.bits(lt) == R.bits(r["low_thr"]), (tt, r["text_thr"], lt, r["low_thr"])
    ref_boxes, ref_conf = hm.detect_boxes(heat, R.TEXT, R.LOW)
    assert len(ref_boxes) == r["n_sel"] == len(r["boxes"])
    if r["n_sel"]:
        assert np.array_equal(np.stack(ref_boxes).astype(np.float32), r["boxes"])
        assert np.array_equal(np.asarray(ref_conf, np.float32), r["conf"])
    boxes, conf, thr = run_native(native, heat, cap=max(4096, r["n_sel"]))
    assert abs(thr[0] - tt) <= 1e-6 and abs(thr[1] - lt) <= 1e-6
    assert len(boxes) == r["n_sel"]
    if r["n_sel"]:
        assert np.abs(boxes - r["boxes"]).max() <= 1e-3
        assert np.allclose(conf, r["conf"], rtol=0, atol=1e-7)


def test_every_mutant_is_killed_by_the_cases_that_list_it():
    listed = set()
    for c in R.CASES:
        for m in c.kills:
            assert m in R.MUTANTS
            stages = R.killed(c.name, m)
            assert stages, f"{c.name} does not kill {m}"
            listed.add(m)
            print(f"{c.name}: {m} differs at {sorted(set(stages))}")
    assert listed == set(R.MUTANTS), set(R.MUTANTS) - listed


def test_pages_reach_what_they_were_drawn_for():
    N = 61 * 68
    assert N == 4148 and int(N * 0.9) != N * 0.9 and 68 % 64 == 4
    for ph in range(3):                                         # the wrap pairs stay apart: two components of area 10 per pair
        r = _full(f"wrap{ph}")
        assert r["n_sel"] == 2 * len(range(ph, 60, 3)) and set(r["area"]) == {10}
    assert {y for ph in range(3) for y in range(ph, 60, 3)} == set(range(60))
    runs = set()                                                # (length, lane of the first pixel) of the runs on the segment pages
    for n in ("segments_s", "segments_a", "segments_r"):
        r = _full(n)
        assert r["n_sel"] == len(r["roots"]) >= 19
        runs |= set(zip(r["area"].tolist(), (r["roots"] % 64).tolist()))
    # across a segment boundary, from lane 63, up to lane 0; 64 / 65 / 128 pixels from lane 0 (aligned) and from elsewhere
    assert {(10, 59), (10, 63), (10, 55), (64, 0), (64, 61), (64, 1), (65, 0), (65, 63), (128, 0), (128, 57)} <= runs, runs
    assert _full("serpentine_s")["n_sel"] == 1 and _full("serpentine_s")["area"][0] == 31 * 68 + 30
    assert _full("checker_s")["n_sel"] == 0 and len(_full("checker_s")["roots"]) == 2074
    d = _full("diagonal_s")
    assert d["n_sel"] == 1 and sorted(set(d["area"])) == [1, 30]            # the staircase only
    for n in ("spiral_s", "spiral_r", "comb_top_s", "comb_bottom_s", "comb_bottom_r"):
        assert len(_full(n)["roots"]) == 1, n
    assert _full("nested_s")["n_sel"] >= 8
    e = _full("equal_s")
    assert e["cnt_gt"] == 0 and e["n_sel"] == 1 and (e["comp"][0]["x0"], e["comp"][0]["x1"], e["comp"][0]["y0"], e["comp"][0]["y1"]) == (0, 67, 0, 60)
    f = _full("filters_a")
    assert R.bits(f["text_thr"]) == R.bits(R.F(0.6)) and R.bits(f["low_thr"]) == R.bits(R.F(0.35))
    assert {9, 10, 11, 12, 13}.issubset(set(f["area"].tolist()))
    assert sorted(f["area"][f["area_final"] < 0].tolist()) == [9, 12]      # what the two filters drop
    sq = _full("squares_a")
    upright = [bool((np.unique(b[:, 0]).size == 2) and (np.unique(b[:, 1]).size == 2)) for b in sq["boxes"]]
    dk = _full("dark_s")
    assert R.bits(dk["text_thr"]) == R.bits(R.F(0.15)) and R.bits(dk["low_thr"]) == R.bits(R.F(0.1)) and dk["n_sel"] == 2 and len(dk["roots"]) == 4
    s = _full("zero_one_s")
    assert s["prefix"] == 0 and R.bits(s["max_conf"]) == 0x3F800000
    p = _full("plateau_a")
    flat = np.sort(R.page("plateau_a").ravel())
    assert (flat == flat[p["k"]]).sum() > 1500 and p["cnt_gt"] == 192 and p["rank"] > 1000
    for n, mask in (("low10_s", 0x3FF), ("mid11_s", 0x7FF << 10)):
        u = R.bits(R.page(n))
        assert len(np.unique(u & ~np.uint32(mask))) == 1 and len(np.unique(u)) > 900, n
    m = _full("many_a")
    assert m["n_sel"] == 320 and R.ref_page(R.page("many_a"), 256)["overflow"] == 1
    a = _full("big_a")
    rows = a["rows"]
    assert 2100 * 516 > 1 << 20 and len(a["blk"]) == 265 and (rows <= R.POST_SMALL_ROWS).sum() > 20
    assert a["blk"][255, 0] > 0 and a["n_sel"] > a["blk"][256, 0] + 10                 # kept components on both sides of the carry
    tall = np.flatnonzero(rows > R.POST_SMALL_ROWS)
    assert len(tall) == 2 and rows[tall].max() == 2100 and max(a["hull_m"]) > 64
    b = _full("big_b")
    cls = sorted({0 if q <= R.POST_SMALL_ROWS else (1 if q <= R.POST_LDS_ROWS else 2) for q in b["rows"].tolist()})
    assert cls == [0, 1, 2] and b["rows"].max() == 2600
    assert sq["n_sel"] == 10 and 2 <= sum(upright) <= 8, upright             # both sides of the near-square rule
    ov = R.reference("overflow")
    assert [p["overflow"] for p in ov[0]] == [0, 1, 0] and [p["overflow"] for p in ov[1]] == [1, 0, 0]


def test_layout_hook_matches_workspace_bytes(hip_lib):
    for B, H, W, mb in ((1, 61, 68, 512), (3, 64, 128, 256), (2, 2600, 68, 512), (1, 2100, 516, 4096), (16, 1024, 1024, 4096)):
        L = R.workspace_layout(hip_lib, B, H, W, mb)
        offs = [L[n] for n in R.LAYOUT_WORDS[:17]] + [L["total"]]
        assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
        assert all(b > a for a, b in zip(offs[:16], offs[1:17])) and offs[17] >= offs[16]
        assert L["total"] == hip_lib.surya_det_boxes_workspace_bytes(B, H, W, mb)
        N = H * W
        assert L["n_blk"] == -(-N // R.SCAN_PIX) and L["row_cap"] == N
        assert L["area"] - L["label"] >= 4 * B * N and L["rmax"] - L["rmin"] >= 4 * B * N and L["rowoff"] - L["comp"] >= 24 * B * mb
        assert (L["big_stride"] > 0) == (H > R.POST_LDS_ROWS) and L["big_stride"] % 256 == 0
        assert L["total"] - L["big"] >= 8 * B * L["big_stride"]
    off = (C.c_size_t * 21)()
    assert hip_lib.surya_det_boxes_workspace_layout(1, 64, 64, 16, off, 20, None, None) == -1          # SA_ERR_ARG: too few words
    assert hip_lib.surya_det_boxes_workspace_layout(0, 64, 64, 16, off, 21, None, None) == -1
    assert hip_lib.surya_det_boxes_workspace_layout(1, 64, 64, 16, None, 21, None, None) == -1
    assert hip_lib.surya_det_boxes_workspace_layout(1, 64, 64, 16, off, 21, None, None) == 0
