"""GPU: the kernels of boosted decoding alone (csrc/boost.h), through surya_op_rec_boost_step / surya_op_rec_boost_head -- the launch code
RecModel uses -- on caller-owned buffers.

boost_step against the host restatement BoostTables.advance / row, on an automaton made by hand: a root with 300 children (more than the
workgroup has lanes), a state with one edge, the state without edges, a second root; 1 / 64 / 320 rows; mask rows of 32 words (vocabulary
1024) and 2560 words (81 920). Every kind of transition: an edge, the fallback to OUT (a word unit without an edge), the fallback to the
slot's root (a boundary without an edge), eos, pad, an id outside the vocabulary, state -1, and a state that stays (OUT behind a word unit).
Exact: states, and every word of the table -- the rows of the slots no row names, the static rows in front and the word row included.

boost_head against csrc/boost_core.h compiled for the host (tests/boost_ref.py; tests/test_boost_cpu.py checks that build against float64)
on hand-made partial records that carry the CPU test's corner cases: token, plain_token and next_token equal; score and plain_prob within
2e-3 (the kernel reduces a row's tiles in another order than the host's float64 sum, and its expf is not the host's). On rows with beta =
+inf token, score and box are bit-identical to surya_op_rec_head on record A; the fused embedding has the bits of
surya_op_rec_decode_embed on the token the head chose."""
import ctypes as C

import numpy as np
import pytest
import torch

import boost_ref as br
from surya_amd import _lib as L
from surya_amd.recognition.boost import BoostTables

pytestmark = pytest.mark.gpu
EOS, PAD = 256, 257
ROW_BASE, WORD_ROW, FREE_STATE = 5, 2, 3            # static rows in front, one of them the word-unit set; the state of slots no row names
OUT, ROOT, ONE, ROOT2, MID = 0, 1, 2, 3, 4
NO_COLUMN = 0x7fffffff
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _automaton(V) -> BoostTables:
    last = V - 1
    edges = {OUT: [],
             ROOT: [(300 + k, ONE if k % 2 == 0 else MID) for k in range(300)],       # 300 children, ten words
             ONE: [(410, OUT)],                                                       # one edge; shares word 12 with ROOT and MID
             ROOT2: [(405, MID), (last, ONE)],                                        # the last id of the last word
             MID: [(400 + k, ROOT2 if k % 3 else OUT) for k in range(26)]}            # 26 children in words 12 and 13
    off, tok, nxt = [0], [], []
    for s in range(5):
        for t, n in edges[s]:
            tok.append(t); nxt.append(n)
        off.append(len(tok))
    word = np.zeros(V, bool)
    word[300:700] = True                                                             # ids 300..699 are "letters", everything else a boundary
    word[last] = True
    return BoostTables(np.asarray(off, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32), [ROOT, ROOT2], OUT, word, {}, V, EOS, PAD)


def _step_case(bt, rows):
    """Per row: its slot, the slot's state and root, and the token its head chose."""
    rng = np.random.default_rng(rows)
    S = rows + 3
    slots = rng.permutation(S)[:rows].astype(np.int32)
    state0, root, token = np.full(S, FREE_STATE, np.int32), np.full(S, ROOT, np.int32), np.full(S, -9, np.int32)
    last = bt.vocab - 1
    kinds = [(ROOT, ROOT, lambda r: 300 + (r * 7) % 300),     # an edge out of 300
             (MID, ROOT, lambda r: 400 + r % 26),             # an edge; old and new set share words
             (ONE, ROOT2, lambda r: 650),                     # a word unit without an edge -> OUT
             (ONE, ROOT2, lambda r: 100),                     # a boundary without an edge -> the slot's root (ROOT2)
             (MID, ROOT, lambda r: 900),                      # ... -> ROOT
             (ROOT2, ROOT2, lambda r: last),                  # the last id
             (ROOT, ROOT, lambda r: EOS), (MID, ROOT, lambda r: PAD), (ONE, ROOT, lambda r: NO_COLUMN), (-1, -1, lambda r: 410),
             (OUT, ROOT, lambda r: 333),                      # OUT stays OUT behind a word unit
             (OUT, ROOT2, lambda r: 5),                       # OUT -> the root behind a boundary
             (ROOT, ROOT, lambda r: 7)]                       # the root stays the root behind a boundary
    for r in range(rows):
        st, rt, t = kinds[r % len(kinds)]
        state0[slots[r]], root[slots[r]], token[slots[r]] = st, rt, t(r)
    return S, slots, state0, root, token


@pytest.mark.parametrize("rows", [1, 64, 320])
@pytest.mark.parametrize("V", [1024, 81920])
def test_step_moves_states_and_rewrites_rows_as_the_host_does(hip_lib, V, rows):
    bt = _automaton(V)
    words = (V + 31) // 32
    S, slots, state0, root, token = _step_case(bt, rows)
    want_tab = np.full((ROW_BASE + S, words), 0xdeadbeef, np.uint32)
    want_tab[WORD_ROW] = bt.word_mask
    for s in range(S):                                       # every slot's row holds its state's set (a slot that is not boosted: garbage)
        if state0[s] >= 0:
            want_tab[ROW_BASE + s] = bt.row(int(state0[s]))
    flags = torch.zeros(bt.n_states, dtype=torch.uint8, device="cuda")
    dev = [torch.from_numpy(x).cuda() for x in (bt.edge_off, bt.edge_tok, bt.edge_next)]
    table = torch.from_numpy(want_tab.view(np.int32).copy()).cuda()
    slot_state, slot_root = torch.from_numpy(state0.copy()).cuda(), torch.from_numpy(root).cuda()
    slot_mask = torch.full((S,), 77, dtype=torch.int32, device="cuda")
    a = L.RecLexiconArgsC()
    a.edge_off, a.edge_tok, a.edge_next = (t.data_ptr() for t in dev)
    a.state_flags, a.table, a.slot_state, a.slot_mask = flags.data_ptr(), table.data_ptr(), slot_state.data_ptr(), slot_mask.data_ptr()
    a.words, a.row_base, a.vocab, a.eos_id, a.pad_id, a.nop_id = words, ROW_BASE, V, EOS, PAD, -1
    d_slots, d_tok = torch.from_numpy(slots).cuda(), torch.from_numpy(token).cuda()
    state = state0.copy()
    for rnd in range(2):                                     # a second step over the same tokens: what can move again does
        assert hip_lib.surya_op_rec_boost_step(C.byref(a), slot_root.data_ptr(), OUT, WORD_ROW, d_slots.data_ptr(), d_tok.data_ptr(), rows, _stream()) == 0
        torch.cuda.synchronize()
        moved = 0
        for s in slots:
            ns = bt.advance(int(state[s]), int(token[s]), int(root[s]))
            if ns != state[s]:
                state[s], want_tab[ROW_BASE + s] = ns, bt.row(ns)
                moved += 1
        assert rnd or moved >= max(1, rows // 2)
        got = table.cpu().numpy().view(np.uint32)
        assert np.array_equal(slot_state.cpu().numpy(), state), (slot_state.cpu().tolist(), state.tolist())
        assert np.array_equal(got, want_tab), np.argwhere(got != want_tab)[:8].tolist()
        assert (slot_mask.cpu().numpy() == 77).all() and np.array_equal(slot_root.cpu().numpy(), root)


def test_the_hand_made_automaton_holds_the_cases():
    """(no GPU work) what the docstring promises about the automaton, on the host restatement."""
    bt = _automaton(81920)
    assert [len(bt.edges(s)[0]) for s in (OUT, ONE, ROOT)] == [0, 1, 300]
    assert {t >> 5 for t in bt.preferred(MID)} == {12, 13} and {t >> 5 for t in bt.preferred(ONE)} == {12}
    assert bt.advance(ONE, 650, ROOT2) == OUT and bt.advance(ONE, 100, ROOT2) == ROOT2 and bt.advance(MID, 900, ROOT) == ROOT
    assert bt.advance(OUT, 333, ROOT) == OUT and bt.advance(ROOT, 7, ROOT) == ROOT and bt.advance(ROOT2, 81919, ROOT2) == ONE


# ------------------------------------------------------------------------------------------------------------------ the head
H, BBOX, TMAX, EPS = 256, 1024, 64, 1e-6


def _tiles(rng, mx, idx, tiles_n, hi):
    """[rows, tiles_n, 4] partial records whose row-level reduction has the maximum `mx` at the first index `idx`: one tile holds it,
    the others sit below (a few exactly AT the maximum with a larger index: the tie goes to the lower id), a few are empty. -> the
    records and the row-level sum in float64."""
    rows = len(mx)
    x = (mx[:, None] - rng.random((rows, tiles_n)) * 9 - 1e-3).astype(np.float32)
    ix = rng.integers(0, hi, (rows, tiles_n)).astype(np.int32)
    z = (1.0 + rng.random((rows, tiles_n)) * 20).astype(np.float32)
    at = rng.integers(0, tiles_n, rows)
    ties = rng.random((rows, tiles_n)) < 0.05
    x[ties] = np.broadcast_to(mx[:, None], x.shape)[ties]
    ix[ties] = (np.broadcast_to(idx[:, None], ix.shape) + 1 + rng.integers(0, 50, ix.shape))[ties]
    gone = rng.random((rows, tiles_n)) < 0.1
    x[gone], ix[gone], z[gone] = -np.inf, br.NONE, 0.0
    r = np.arange(rows)
    x[r, at], ix[r, at] = mx, idx
    z[r, at] = np.where(np.isfinite(mx), 1.0 + rng.random(rows) * 20, 0.0)
    empty = ~np.isfinite(mx)
    x[empty], ix[empty], z[empty] = -np.inf, br.NONE, 0.0
    with np.errstate(invalid="ignore"):
        tot = np.where(empty, 0.0, (z.astype(np.float64) * np.exp(np.where(np.isfinite(x), x.astype(np.float64) - mx[:, None], -np.inf))).sum(axis=1))
    part = np.zeros((rows, tiles_n, 4), np.float32)
    part[..., 0], part[..., 2] = x, z
    part[..., 1] = ix.view(np.float32)
    return part, tot


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("tiles_n", [1, 5, 218, 256])
@pytest.mark.parametrize("rows", [1, 64, 320])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_head_against_the_host_core(hip_lib, dtype, rows, tiles_n, fused):
    rng = np.random.default_rng(rows * 1000 + tiles_n)
    V = 5000
    maxA, idxA, _, maxB, idxB, _, beta = br.edge_records(rng, rows)
    idxA[np.isfinite(maxA)] = np.minimum(idxA[np.isfinite(maxA)], V - 60)
    idxB = np.minimum(idxB, V - 60)
    if rows > 8:
        idxB[3], maxB[3], maxA[3], idxA[3], beta[3] = EOS, 5.0, 1.0, 40, 0.0          # a row that ends: score 0, next token pad
        idxA[4], maxA[4], beta[4] = PAD, maxB[4] - 1.0, 80.0                          # ... through the boost
    part_a, sumA = _tiles(rng, maxA, idxA, tiles_n, V)
    part_b, sumB = _tiles(rng, maxB, idxB, tiles_n, V)
    token, tot, ptok, pprob = br.native_combine(maxA, idxA, sumA.astype(np.float32), maxB, idxB, sumB.astype(np.float32), beta)
    S = rows + 3
    slots = rng.permutation(S)[:rows].astype(np.int32)
    g = torch.Generator().manual_seed(rows + tiles_n)
    hidden, wb, bb = (torch.randn(s, generator=g).to(dtype).cuda() for s in ((rows, H), (6, H), (6,)))
    table, wnorm = torch.randn((V, H), generator=g).to(dtype).cuda(), torch.rand((H,), generator=g).add(0.5).to(dtype).cuda()
    kv0 = torch.from_numpy(rng.integers(1, TMAX + 4, S).astype(np.int32))
    d_slots = torch.from_numpy(slots).cuda()
    d_a, d_b = torch.from_numpy(part_a).cuda(), torch.from_numpy(part_b).cuda()
    # the plain head is never given a row without a column (its token would be the "no column" index, which the fused embedding would
    # look up): for the comparison run such rows carry record B
    part_p = part_a.copy()
    part_p[~np.isfinite(maxA)] = part_b[~np.isfinite(maxA)]
    d_p = torch.from_numpy(part_p).cuda()
    slot_beta = torch.full((S,), float("nan"))
    slot_beta[torch.from_numpy(slots).long()] = torch.from_numpy(beta)
    slot_beta = slot_beta.cuda()

    def run(boosted):
        o = dict(out_token=torch.full((S,), -5, dtype=torch.int32), out_score=torch.full((S,), -5.0), out_bbox=torch.full((S, 6), -5, dtype=torch.int32),
                 next_token=torch.full((S,), -5, dtype=torch.int32), kv_len=kv0.clone(), plain_token=torch.full((S,), -5, dtype=torch.int32),
                 plain_prob=torch.full((S,), -5.0), row_len=torch.full((rows,), -5, dtype=torch.int32),
                 x=torch.full((rows, H), 7.0).to(dtype), y=torch.full((rows, H), 7.0).to(dtype))
        o = {k: v.cuda() for k, v in o.items()}
        ba = L.RecBoostHeadArgsC()
        a = ba.head
        a.part, a.hidden, a.wb, a.bb, a.row_slot = (d_a if boosted else d_p).data_ptr(), hidden.data_ptr(), wb.data_ptr(), bb.data_ptr(), d_slots.data_ptr()
        for k in ("out_token", "out_score", "out_bbox", "next_token", "kv_len"):
            setattr(a, k, o[k].data_ptr())
        a.tiles_n, a.rows, a.H, a.eos_id, a.pad_id, a.len_inc, a.max_kv_len, a.srows = tiles_n, rows, H, EOS, PAD, 1, TMAX, S
        a.bbox_size, a.eps = float(BBOX), EPS
        if fused:
            a.table, a.wnorm, a.x, a.y, a.row_len = table.data_ptr(), wnorm.data_ptr(), o["x"].data_ptr(), o["y"].data_ptr(), o["row_len"].data_ptr()
        if boosted:
            ba.part_b, ba.slot_beta = d_b.data_ptr(), slot_beta.data_ptr()
            ba.plain_token, ba.plain_prob = o["plain_token"].data_ptr(), o["plain_prob"].data_ptr()
            rc = hip_lib.surya_op_rec_boost_head(DT[dtype], C.byref(ba), _stream())
        else:
            rc = hip_lib.surya_op_rec_head(DT[dtype], C.byref(a), _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        return {k: v.cpu() for k, v in o.items()}

    o = run(True)
    sl = torch.from_numpy(slots).long()
    got_tok, got_ptok = o["out_token"][sl].numpy(), o["plain_token"][sl].numpy()
    assert np.array_equal(got_tok, token), np.flatnonzero(got_tok != token)[:8].tolist()
    assert np.array_equal(got_ptok, ptok)
    done = (token == EOS) | (token == PAD)
    assert np.array_equal(o["next_token"][sl].numpy(), np.where(done, PAD, token))
    want_score = np.where(done, 0.0, 1.0 / tot.astype(np.float64))
    e_s = np.abs(o["out_score"][sl].numpy() / np.where(done, 1.0, want_score) - np.where(done, 0.0, 1.0)).max()
    e_p = np.abs(o["plain_prob"][sl].numpy() / pprob.astype(np.float64) - 1).max()
    print(f"BOOSTHEAD {dtype} rows {rows} tiles {tiles_n}: score rel {e_s:.3g}, plain_prob rel {e_p:.3g}")
    assert e_s <= 2e-3 and e_p <= 2e-3
    assert np.array_equal(o["kv_len"][sl].numpy(), kv0[sl].numpy() + 1)
    other = np.setdiff1d(np.arange(S), slots)
    for k in ("out_token", "next_token", "plain_token"):                  # slots no row names are untouched
        assert (o[k][other] == -5).all()
    assert (o["kv_len"][other] == kv0[other]).all() and (o["out_bbox"][other] == -5).all()
    # beta = +inf: record A alone, the bits of the plain head on it; the box does not depend on the records at all
    p = run(False)
    inf = np.isinf(beta) & np.isfinite(maxA)
    assert rows < 8 or inf.sum() > 3
    si = sl[torch.from_numpy(inf)]
    assert torch.equal(o["out_token"][si], p["out_token"][si])
    assert torch.equal(o["out_score"][si].view(torch.int32), p["out_score"][si].view(torch.int32))
    assert torch.equal(o["out_bbox"], p["out_bbox"]) and (o["out_bbox"][sl] >= 0).all()
    if fused:
        # the fused tail: the bits surya_op_rec_decode_embed gives for the token the head chose
        x2, y2 = torch.full((rows, H), 3.0).to(dtype).cuda(), torch.full((rows, H), 3.0).to(dtype).cuda()
        rl2 = torch.full((rows,), -1, dtype=torch.int32).cuda()
        nt, kv = o["next_token"].cuda(), o["kv_len"].cuda()
        rc = hip_lib.surya_op_rec_decode_embed(DT[dtype], table.data_ptr(), nt.data_ptr(), d_slots.data_ptr(), kv.data_ptr(), TMAX, rl2.data_ptr(),
                                               x2.data_ptr(), wnorm.data_ptr(), y2.data_ptr(), rows, H, EPS, None, None, 0, _stream())
        torch.cuda.synchronize()
        assert rc == 0
        assert torch.equal(o["x"].view(torch.uint8), x2.cpu().view(torch.uint8)) and torch.equal(o["y"].view(torch.uint8), y2.cpu().view(torch.uint8))
        assert torch.equal(o["row_len"], rl2.cpu())
        assert torch.equal(o["x"], table.cpu()[torch.from_numpy(np.where(done, PAD, token)).long()])
    else:
        assert (o["x"] == 7).all() and (o["row_len"] == -5).all()


def test_op_hooks_refuse_incomplete_operands(hip_lib):
    x = torch.zeros(8192, dtype=torch.int32, device="cuda")
    p, s = x.data_ptr(), _stream()
    a = L.RecLexiconArgsC()
    a.edge_off = a.edge_tok = a.edge_next = a.state_flags = a.table = a.slot_state = a.slot_mask = p
    a.words, a.row_base, a.vocab = 4, 0, 128
    assert hip_lib.surya_op_rec_boost_step(C.byref(a), None, 0, 0, p, p, 1, s) == L.SA_ERR_ARG           # no roots
    assert hip_lib.surya_op_rec_boost_step(C.byref(a), p, -1, 0, p, p, 1, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_boost_step(C.byref(a), p, 0, 0, None, p, 1, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_boost_step(C.byref(a), p, 0, 0, p, p, 0, s) == 0                         # no rows: nothing to launch
    ba = L.RecBoostHeadArgsC()
    h = ba.head
    for k in ("part", "hidden", "wb", "bb", "row_slot", "out_token", "out_score", "out_bbox", "next_token", "kv_len"):
        setattr(h, k, p)
    h.tiles_n, h.rows, h.H, h.max_kv_len = 4, 1, 128, 8
    ba.part_b = ba.slot_beta = ba.plain_token = p                                                        # plain_prob missing
    assert hip_lib.surya_op_rec_boost_head(L.DTYPE_F32, C.byref(ba), s) == L.SA_ERR_ARG
    ba.plain_prob = p
    h.best_tot = p                                                                                       # alternatives are refused beside boosting
    assert hip_lib.surya_op_rec_boost_head(L.DTYPE_F32, C.byref(ba), s) == L.SA_ERR_ARG
    h.best_tot = None
    h.tiles_n = 4 * 384 + 1                                                                              # where the fallback head would run
    assert hip_lib.surya_op_rec_boost_head(L.DTYPE_F32, C.byref(ba), s) == L.SA_ERR_STATE
    L.check(hip_lib.surya_set_tuning(b"ghead", C.c_int(1)), "surya_set_tuning")
    try:
        h.tiles_n = 4
        assert hip_lib.surya_op_rec_boost_head(L.DTYPE_F32, C.byref(ba), s) == L.SA_ERR_STATE
    finally:
        L.check(hip_lib.surya_set_tuning(b"ghead", C.c_int(2)), "surya_set_tuning")
    assert hip_lib.surya_op_rec_boost_head(9, C.byref(ba), s) != 0
    torch.cuda.synchronize()
