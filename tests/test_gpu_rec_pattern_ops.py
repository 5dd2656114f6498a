"""GPU: the automaton step of pattern-guided decoding inside the greedy heads, alone, through surya_op_rec_head (the launcher
RecModel::heads uses): greedy_head2_kernel (Tuning ghead = 2), with and without the fused next-step embedding, and the fallback
greedy_head_kernel<T, true> (ghead = 1), in fp32 / bf16 / fp16, 1 / 64 / 320 rows, H = 256.

The lm_head partials are made by hand, so the token every row chooses is known: one tile holds the row's maximum and names the token. The
tables are compiled from real patterns (recognition/pattern.py) over REC-SMALL's vocabulary. After the launch slot_state / slot_mask must
equal PatternTables.advance, the host restatement: ordinary tokens move, eos / pad rows keep their state, slots with state -1 and slots no
row names keep their (sentinel) entries. With the pattern pointers NULL, or every state -1, every other output is bit-identical."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from surya_amd import _lib as L
from surya_amd.config import rec_config

pytestmark = pytest.mark.gpu
H, TILES, TMAX = 256, 7, 64
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
PATTERNS = [r"\d{2}/\d{2}/\d{4}", r"-?\d{1,3}(,\d{3})*\.\d{2}", r"[A-Z]{2}\d{2}( ?[A-Z0-9]{4}){2,7}"]
MASK_SENT, FREE_STATE = 77, 5            # slot_mask entries before the launch; the state of slots no row names


@functools.lru_cache(maxsize=None)
def _tables():
    from surya_amd.recognition.loader import RecognitionModelLoader
    from surya_amd.recognition.pattern import compile_patterns
    cfg = rec_config("REC-SMALL")
    tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
    return cfg, compile_patterns(tk, PATTERNS, cfg.decoder.vocab_size)


def _first_allowed(pt, state, skip):
    """The lowest text id allowed in `state` (an ASCII one for these patterns), or None where the state allows eos / pad only."""
    row = pt.table.rows[int(pt.state_mask[state])]
    ids = np.flatnonzero(np.unpackbits(row.view(np.uint8), bitorder="little"))
    ids = [int(i) for i in ids if int(i) not in skip]
    return ids[0] if ids else None


def _case(rows, seed):
    """Per row: slot, start state, chosen token; and what the host says the entries are afterwards."""
    cfg, pt = _tables()
    rng = np.random.default_rng(seed)
    S = rows + 3
    slots = rng.permutation(S)[:rows].astype(np.int32)
    state0 = np.full(S, FREE_STATE, np.int32)
    tok = np.zeros(rows, np.int64)
    for r in range(rows):
        kind = r % 8
        st = -1 if kind == 3 else (r * 7) % pt.n_states
        t = _first_allowed(pt, max(st, 0), (cfg.eos_token_id, cfg.pad_token_id, pt.nop))
        if kind == 1 or t is None:
            t = cfg.eos_token_id                                   # a row that ends keeps its state
        elif kind == 5:
            t = cfg.pad_token_id
        elif kind == 6:
            t = pt.nop                                             # the no-output id (dead class): the state's own row again
        state0[slots[r]] = st
        tok[r] = t
    state1, mask1 = state0.copy(), np.full(S, MASK_SENT, np.int32)
    for r in range(rows):
        s, st = slots[r], int(state0[slots[r]])
        if st >= 0 and tok[r] not in (cfg.eos_token_id, cfg.pad_token_id):
            ns = pt.advance(st, int(tok[r]))
            state1[s], mask1[s] = ns, int(pt.state_mask[ns])
        else:
            assert pt.advance(st, int(tok[r])) == st
    assert (state1 != state0).sum() >= max(1, rows // 4) or rows == 1
    return S, slots, state0, tok, state1, mask1


def _operands(rows, tok, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    part = torch.zeros(rows, TILES, 4)
    part[:, :, 0] = torch.rand(rows, TILES, generator=g) * 2 - 3           # tile maxima below the winner's
    part[:, :, 2] = torch.rand(rows, TILES, generator=g) * 3 + 1           # sums of exp
    idx = torch.randint(0, 60000, (rows, TILES), generator=g, dtype=torch.int32)
    win = torch.arange(rows) % TILES
    part[torch.arange(rows), win, 0] = 5.0
    idx[torch.arange(rows), win] = torch.from_numpy(tok).int()
    part[:, :, 1] = idx.view(torch.float32)
    hidden = (torch.randn(rows, H, generator=g) * 0.5).to(dtype)
    wb, bb = (torch.randn(6, H, generator=g) * 0.1).to(dtype), torch.randn(6, generator=g).to(dtype)
    n_emb = int(tok.max()) + 1
    table, wnorm = (torch.randn(n_emb, H, generator=g) * 0.3).to(dtype), (1 + 0.1 * torch.randn(H, generator=g)).to(dtype)
    return [t.cuda().contiguous() for t in (part, hidden, wb, bb, table, wnorm)]


def _launch(lib, dtype, rows, S, slots, ops, fused, pattern, state0):
    """One head launch; `pattern`: None (NULL pointers) or the device tables. -> every output as host arrays."""
    cfg, _ = _tables()
    part, hidden, wb, bb, table, wnorm = ops
    i32 = dict(dtype=torch.int32, device="cuda")
    o = dict(out_token=torch.full((S,), -9, **i32), out_score=torch.full((S,), -9.0, device="cuda"), out_bbox=torch.full((S, 6), -9, **i32),
             next_token=torch.full((S,), -9, **i32), kv_len=torch.arange(S, **i32) % 40 + 3)
    row_slot = torch.from_numpy(slots).cuda()
    a = L.RecHeadArgsC()
    a.part, a.hidden, a.wb, a.bb, a.row_slot = (t.data_ptr() for t in (part, hidden, wb, bb, row_slot))
    a.tiles_n, a.rows, a.H, a.eos_id, a.pad_id, a.len_inc = TILES, rows, H, cfg.eos_token_id, cfg.pad_token_id, 1
    a.max_kv_len, a.srows, a.bbox_size, a.eps = TMAX, S, float(cfg.bbox_size), 1e-6
    if fused:
        o.update(row_len=torch.full((rows,), -9, **i32), x=torch.full((rows, H), 7.0, device="cuda").to(dtype),
                 y=torch.full((rows, H), 7.0, device="cuda").to(dtype))
        a.table, a.wnorm, a.x, a.y, a.row_len = (t.data_ptr() for t in (table, wnorm, o["x"], o["y"], o["row_len"]))
    if pattern is not None:
        tc, ns, sm, n_classes = pattern
        o.update(slot_state=torch.from_numpy(state0).cuda(), slot_mask=torch.full((S,), MASK_SENT, **i32))
        a.pat_tok_class, a.pat_next_state, a.pat_state_mask = tc.data_ptr(), ns.data_ptr(), sm.data_ptr()
        a.pat_slot_state, a.pat_slot_mask, a.pat_n_classes, a.pat_vocab = o["slot_state"].data_ptr(), o["slot_mask"].data_ptr(), n_classes, tc.numel()
    for k in ("out_token", "out_score", "out_bbox", "next_token", "kv_len"):
        setattr(a, k, o[k].data_ptr())
    rc = lib.surya_op_rec_head(DT[dtype], C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {k: (v.view(torch.int16) if v.dtype in (torch.bfloat16, torch.float16) else v).cpu().numpy() for k, v in o.items()}


@pytest.fixture
def ghead(hip_lib):
    def set_(v):
        L.check(hip_lib.surya_set_tuning(b"ghead", C.c_int(v)), "surya_set_tuning(ghead)")
    yield set_
    set_(2)


@pytest.mark.parametrize("rows", [1, 64, 320])
@pytest.mark.parametrize("kernel", ["head2", "head2-fused", "fallback"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_head_advances_the_automaton_as_the_host_does(hip_lib, ghead, dtype, kernel, rows):
    cfg, pt = _tables()
    ghead(1 if kernel == "fallback" else 2)
    fused = kernel == "head2-fused"
    S, slots, state0, tok, state1, mask1 = _case(rows, seed=rows)
    ops = _operands(rows, tok, dtype, seed=rows + 1)
    dev = (torch.from_numpy(pt.tok_class).cuda(), torch.from_numpy(pt.next_state.view(np.int16)).cuda(), torch.from_numpy(pt.state_mask).cuda(),
           pt.n_classes)
    plain = _launch(hip_lib, dtype, rows, S, slots, ops, fused, None, state0)
    assert np.array_equal(plain["out_token"][slots], tok), "the hand-made partials do not choose the intended tokens"
    got = _launch(hip_lib, dtype, rows, S, slots, ops, fused, dev, state0)
    assert np.array_equal(got["slot_state"], state1), (got["slot_state"].tolist(), state1.tolist())
    assert np.array_equal(got["slot_mask"], mask1), (got["slot_mask"].tolist(), mask1.tolist())
    for k, v in plain.items():                                     # tokens, scores, boxes, the next input and the fused embedding: the same bits
        assert np.array_equal(v.view(np.uint8), got[k].view(np.uint8)), k
    # every slot without a pattern: nothing is written, nothing else changes
    off = _launch(hip_lib, dtype, rows, S, slots, ops, fused, dev, np.full(S, -1, np.int32))
    assert (off["slot_state"] == -1).all() and (off["slot_mask"] == MASK_SENT).all()
    for k, v in plain.items():
        assert np.array_equal(v.view(np.uint8), off[k].view(np.uint8)), k


def test_head_refuses_incomplete_pattern_operands(hip_lib):
    x = torch.zeros(4096, device="cuda")
    p = x.data_ptr()
    a = L.RecHeadArgsC()
    for k in ("part", "hidden", "wb", "bb", "row_slot", "out_token", "out_score", "out_bbox", "next_token", "kv_len"):
        setattr(a, k, p)
    a.tiles_n, a.rows, a.H, a.max_kv_len = 4, 1, 128, 8
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a.pat_tok_class = p                                             # the other four pointers missing
    assert hip_lib.surya_op_rec_head(L.DTYPE_F32, C.byref(a), s) == L.SA_ERR_ARG
    a.pat_next_state = a.pat_state_mask = a.pat_slot_state = a.pat_slot_mask = p
    a.pat_n_classes, a.pat_vocab = 257, 16                          # more classes than a uint8 names
    assert hip_lib.surya_op_rec_head(L.DTYPE_F32, C.byref(a), s) == L.SA_ERR_ARG
    a.pat_n_classes = 4
    a.forced_table = a.forced_cursor = a.flogit = a.greedy_token = a.greedy_prob = a.logprob = p
    a.forced_stride = 4                                             # not beside forced decoding
    assert hip_lib.surya_op_rec_head(L.DTYPE_F32, C.byref(a), s) == L.SA_ERR_ARG
    torch.cuda.synchronize()
