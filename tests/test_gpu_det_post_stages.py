"""GPU: every stage of surya_det_boxes (csrc/det_post.h) against the staged reference of tests/det_post_ref.py, on adversarial maps.

One call per case, then the caller-owned workspace is read through surya_det_boxes_workspace_layout and EVERY element of every stage is
held to the reference: the radix select's PageState, the label of every pixel, the statistics at every root, the scan blocks, the
component table, the row-extreme slices, and the boxes. Integers are held exactly; the only tolerances are sum_gt (N 2^-52 sum against
fsum: N float64 additions in any order), avg (one float32 step: a rounded float64 quotient rounded again) and the existing bar of the final
boxes (corners 1e-3 px, confidences 1e-7: test_gpu_det_post.py). Every call runs with page_stride = 2 H W + 8 and NaN in everything
between the pages, a workspace of 0xA5 bytes and sentinel outputs. All inputs are inside the documented contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import det_post_ref as R

pytestmark = pytest.mark.gpu


def _call(lib, pages, max_boxes, ws=None, stride_extra=None, heat_offset=0, ws_short=0):
    """One surya_det_boxes call. Returns everything that was on the device afterwards, as numpy."""
    B = len(pages)
    H, W = pages[0].shape
    N = H * W
    stride = 2 * N + 8 if stride_extra is None else N + stride_extra
    buf = np.full(B * stride + 4, np.nan, np.float32)
    for b, m in enumerate(pages):
        buf[b * stride: b * stride + N] = m.ravel()
    heat = torch.from_numpy(buf).cuda()
    need = int(lib.surya_det_boxes_workspace_bytes(C.c_int(B), C.c_int(H), C.c_int(W), C.c_int(max_boxes)))
    if ws is None:
        ws = torch.full((need,), R.WS_FILL, dtype=torch.uint8, device="cuda")
    boxes = torch.full((B, max_boxes, 4, 2), float(R.SENT), dtype=torch.float32, device="cuda")
    conf = torch.full((B, max_boxes), float(R.SENT), dtype=torch.float32, device="cuda")
    count = torch.full((B,), R.SENT_COUNT, dtype=torch.int32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.surya_det_boxes(C.c_void_p(heat.data_ptr() + heat_offset), C.c_long(stride), C.c_int(B), C.c_int(H), C.c_int(W), C.c_float(R.TEXT),
                             C.c_float(R.LOW), C.c_int(max_boxes), C.c_void_p(boxes.data_ptr()), C.c_void_p(conf.data_ptr()),
                             C.c_void_p(count.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(need - ws_short), stream)
    torch.cuda.synchronize()
    return dict(rc=rc, B=B, H=H, W=W, N=N, max_boxes=max_boxes, ws_t=ws, ws=ws.cpu().numpy(), heat_before=buf, heat_after=heat.cpu().numpy(),
                boxes=boxes.cpu().numpy(), conf=conf.cpu().numpy(), count=count.cpu().numpy(),
                L=R.workspace_layout(lib, B, H, W, max_boxes) if W % 4 == 0 else None)


def _arr(out, word, dtype, per_page):
    """[B][per_page] view of one workspace array."""
    n = out["B"] * per_page
    dt = np.dtype(dtype)
    o = out["L"][word]
    return out["ws"][o: o + n * dt.itemsize].view(dt).reshape(out["B"], per_page)


def _stages(out):
    """Every array one call defines, per page: what a second call on the same workspace must reproduce bit for bit."""
    N, mb, L = out["N"], out["max_boxes"], out["L"]
    sweep = min(1024, -(-N // 1024))
    st = _arr(out, "st", R.PAGE_STATE_DT, 1)[:, 0]
    d = dict(st=st, hist=_arr(out, "hist", "<u4", 2048), psum=_arr(out, "psum", "<u8", 1024)[:, :sweep], pcnt=_arr(out, "pcnt", "<u4", 1024)[:, :sweep],
             blk=_arr(out, "blk", "<i4", 2 * L["n_blk"]).reshape(out["B"], L["n_blk"], 2))
    for w in ("label", "area", "minx", "maxx", "miny", "maxy"):
        d[w] = _arr(out, w, "<i4", N)
    d["maxv"] = _arr(out, "maxv", "<u4", N)
    comp, rowoff = _arr(out, "comp", R.COMP_DT, mb), _arr(out, "rowoff", "<i4", mb)
    rmin, rmax = _arr(out, "rmin", "<i4", L["row_cap"]), _arr(out, "rmax", "<i4", L["row_cap"])
    d["comp"], d["rowoff"], d["rmin"], d["rmax"] = [], [], [], []
    for b in range(out["B"]):
        n_sel = 0 if st[b]["overflow"] else max(0, min(int(st[b]["n_sel"]), mb))
        n_rows = 0 if st[b]["overflow"] else max(0, min(int(st[b]["n_rows"]), L["row_cap"]))
        d["comp"].append(comp[b, :n_sel]); d["rowoff"].append(rowoff[b, :n_sel])
        d["rmin"].append(rmin[b, :n_rows]); d["rmax"].append(rmax[b, :n_rows])
    d.update(boxes=out["boxes"], conf=out["conf"], count=out["count"])
    return d


def _same_bits(a, b):
    if isinstance(a, list):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_page(out, d, b, ref, name):
    """Page b of one call against its reference, stage by stage."""
    N = out["N"]
    tag = f"{name} (page {b})"
    st = d["st"][b]
    # 1. the select and the thresholds
    k = ref["k"]
    assert int(st["prefix"]) == ref["prefix"], (tag, hex(int(st["prefix"])), hex(ref["prefix"]))
    assert int(st["rank"]) == ref["rank"], tag
    assert int(st["cnt_gt"]) == ref["cnt_gt"], (tag, int(st["cnt_gt"]), ref["cnt_gt"])
    assert int(d["pcnt"][b].sum()) == ref["cnt_gt"], tag
    assert abs(float(st["sum_gt"]) - ref["sum_gt"]) <= N * 2.0 ** -52 * ref["sum_gt"], (tag, float(st["sum_gt"]), ref["sum_gt"])
    assert not d["hist"][b].any(), tag                                   # the last pick leaves the histogram cleared
    vk = float(np.uint32(st["prefix"]).view(np.float32))
    avg = R.F((float(st["sum_gt"]) + float(N - k - int(st["cnt_gt"])) * vk) / float(N - k))
    assert abs(float(avg) - float(ref["avg"])) <= R.f32_step(ref["avg"]), (tag, avg, ref["avg"])
    tt, lt = R.thr_formula(avg)
    assert R.bits(st["text_thr"]) == R.bits(tt) and R.bits(st["low_thr"]) == R.bits(lt), (tag, st["text_thr"], tt, st["low_thr"], lt)
    if name not in R.NON_DYADIC:
        assert R.bits(st["text_thr"]) == R.bits(ref["text_thr"]) and R.bits(st["low_thr"]) == R.bits(ref["low_thr"]), tag
    # 2. labels and root statistics
    bad = np.flatnonzero(d["label"][b] != ref["label"])
    assert bad.size == 0, (tag, "label", bad.size, [(int(i), int(d["label"][b][i]), int(ref["label"][i])) for i in bad[:8]])
    roots = ref["roots"]
    for w in ("minx", "maxx", "miny", "maxy", "maxv"):
        got = d[w][b][roots]
        assert np.array_equal(got, ref[w]), (tag, w, [(int(roots[i]), int(got[i]), int(ref[w][i])) for i in np.flatnonzero(got != ref[w])[:8]])
    got = d["area"][b][roots]
    assert np.array_equal(got, ref["area_final"]), (tag, "area", [(int(roots[i]), int(got[i]), int(ref["area_final"][i]))
                                                                  for i in np.flatnonzero(got != ref["area_final"])[:8]])
    rest = d["area"][b].copy()
    rest[roots] = 0
    assert not rest.any(), (tag, "area off the roots")
    # 3. selection
    assert (int(st["n_sel"]), int(st["n_rows"]), int(st["overflow"])) == (ref["n_sel"], ref["n_rows"], ref["overflow"]), tag
    assert np.array_equal(d["blk"][b], ref["blk"]), (tag, "blk", np.flatnonzero((d["blk"][b] != ref["blk"]).any(1))[:8])
    box, conf = out["boxes"][b], out["conf"][b]
    if ref["overflow"]:
        assert out["count"][b] == -1, tag
        assert R.bits(st["max_conf"]) == 0, tag
        assert (box == R.SENT).all() and (conf == R.SENT).all(), (tag, "an overflowing page wrote an output")
        return
    assert R.bits(st["max_conf"]) == R.bits(ref["max_conf"]), tag
    for f in ("x0", "x1", "y0", "y1", "area"):
        assert np.array_equal(d["comp"][b][f], ref["comp"][f]), (tag, "comp", f)
    assert np.array_equal(R.bits(d["comp"][b]["maxv"]), R.bits(ref["comp"]["maxv"])), (tag, "comp maxv")
    assert np.array_equal(d["rowoff"][b], ref["rowoff"]), (tag, "rowoff")
    for w in ("rmin", "rmax"):
        bad = np.flatnonzero(d[w][b] != ref[w])
        assert bad.size == 0, (tag, w, bad.size, [(int(i), int(d[w][b][i]), int(ref[w][i])) for i in bad[:8]])
    # 4. boxes
    n = ref["n_sel"]
    assert out["count"][b] == n, (tag, out["count"][b], n)
    if n:
        err = np.abs(box[:n] - ref["boxes"]).reshape(n, -1).max(1)
        assert err.max() <= 1e-3, (tag, "boxes", int(err.argmax()), float(err.max()), box[int(err.argmax())], ref["boxes"][int(err.argmax())])
        assert np.abs(conf[:n] - ref["conf"]).max() <= 1e-7, (tag, "conf")
    assert (box[n:] == R.SENT).all() and (conf[n:] == R.SENT).all(), (tag, "written past count")


def _check_call(out, refs, names):
    assert out["rc"] == 0, out["rc"]
    assert out["heat_before"].tobytes() == out["heat_after"].tobytes(), "the heat buffer changed"
    d = _stages(out)
    for b, (ref, name) in enumerate(zip(refs, names)):
        _check_page(out, d, b, ref, name)
    return d


@pytest.mark.parametrize("case", [c.name for c in R.CASES])
def test_every_stage_of_one_call(hip_lib, case):
    c = R.CASE_BY_NAME[case]
    refs = R.reference(case)
    out = _call(hip_lib, [R.page(n) for n in c.pages], c.max_boxes)
    _check_call(out, refs[0], c.pages)
    assert [b for b in range(len(c.pages)) if out["count"][b] == -1] == list(c.overflows)
    if c.second:                                    # other maps on the workspace the first call used
        out2 = _call(hip_lib, [R.page(n) for n in c.second], c.max_boxes, ws=out["ws_t"])
        _check_call(out2, refs[1], c.second)


@pytest.mark.parametrize("case", [c.name for c in R.CASES if c.second] + ["big_b"])
def test_used_workspace_and_repeat_are_bit_identical(hip_lib, case):
    """A call on a workspace another call used == the same call on a fresh (0xA5) workspace == the same call again, in every byte a call
    defines (_stages)."""
    c = R.CASE_BY_NAME[case]
    first, then = [R.page(n) for n in c.pages], [R.page(n) for n in (c.second or c.pages)]
    used = _call(hip_lib, first, c.max_boxes)
    again = _stages(_call(hip_lib, then, c.max_boxes, ws=used["ws_t"]))
    once_more = _stages(_call(hip_lib, then, c.max_boxes, ws=used["ws_t"]))
    fresh = _stages(_call(hip_lib, then, c.max_boxes))
    for key in fresh:
        assert _same_bits(fresh[key], again[key]), (case, key, "used workspace")
        assert _same_bits(fresh[key], once_more[key]), (case, key, "repeat")


@pytest.mark.parametrize("case,mutant", [(c.name, m) for c in R.CASES for m in c.kills])
def test_the_checks_reject_every_mutant(hip_lib, case, mutant):
    """The other direction: what the device left, held to a deliberately wrong reference, must not pass (the checks above look at the
    stage each mutant moves)."""
    c = R.CASE_BY_NAME[case]
    wrong = R.reference(case, mutant)
    outs = [_call(hip_lib, [R.page(n) for n in c.pages], c.max_boxes)]
    if c.second:
        outs.append(_call(hip_lib, [R.page(n) for n in c.second], c.max_boxes, ws=outs[0]["ws_t"]))
    rejected = False
    for out, refs, names in zip(outs, wrong, (c.pages, c.second)):
        try:
            _check_call(out, refs, names)
        except AssertionError:
            rejected = True
    assert rejected, (case, mutant)


def test_refusals_write_nothing(hip_lib):
    """Each documented refusal returns its error before anything is enqueued: workspace, boxes, confidences and counts keep their fill."""
    ok = np.full((8, 8), 0.5, np.float32)
    for what, kw, pages, want in (("W % 4", {}, [np.full((8, 6), 0.5, np.float32)], -2),
                                  ("page_stride % 4", dict(stride_extra=2), [ok, ok], -2),
                                  ("heat off 16 bytes", dict(heat_offset=4), [ok], -2),
                                  ("workspace one byte short", dict(ws_short=1), [ok], -5)):
        out = _call(hip_lib, pages, 16, **kw)
        assert out["rc"] == want, (what, out["rc"])
        assert (out["ws"] == R.WS_FILL).all(), what
        assert (out["boxes"] == R.SENT).all() and (out["conf"] == R.SENT).all() and (out["count"] == R.SENT_COUNT).all(), what
        assert out["heat_before"].tobytes() == out["heat_after"].tobytes(), what
    assert _call(hip_lib, [ok], 16)["rc"] == 0                  # the same call without any of them is accepted
