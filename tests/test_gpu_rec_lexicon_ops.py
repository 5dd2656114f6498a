"""GPU: the two kernels of lexicon-guided decoding alone (csrc/lexicon.h), through surya_op_rec_lexicon_start / surya_op_rec_lexicon_step --
the launch code RecModel uses -- on caller-owned buffers, against the host restatement LexiconTables.allowed / advance.

1 / 64 / 320 rows; rows of 32 words (vocabulary 1024) and 2560 words (81 920). The automaton is made by hand and holds what can go
wrong: a state with 300 children (more than the workgroup has lanes), a state whose 26 children share two words (lost bits without the
atomic), transitions whose old and new sets share a word (the barrier between clearing and setting), a terminal leaf, a child at the
vocabulary's last id in the row's last word, a state with an edge to itself (the step kernel returns early there: state and row stay, as
the host restatement says). Rows that ended (eos, pad), rows with state -1, a row whose token is the head's "no column"
index and the no-output token at the start state must touch nothing. The start runs onto a table filled with 0xff.

Exact: a touched slot's row equals the new state's set bit for bit, every other word zero; untouched slots' rows, states and mask ids, and
the static rows in front, are bit-identical to before; states equal advance."""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L
from surya_amd.recognition.lexicon import LexiconTables

pytestmark = pytest.mark.gpu
EOS, PAD, NOP = 256, 257, 264
ROW_BASE, MASK_SENT, FREE_STATE = 5, 77, 3          # static rows in front; slot_mask before the start; the state of slots no row names
ROOT, A, B, CC, LEAF, LOOP = 0, 1, 2, 3, 4, 5
NO_COLUMN = 0x7fffffff


def _automaton(V) -> LexiconTables:
    last = V - 1
    edges = {ROOT: [(300 + k, A if k % 2 == 0 else B) for k in range(300)],         # 300 children, ten words
             A: [(400 + k, B if k % 3 else LEAF) for k in range(26)],                # 26 children in words 12 and 13
             B: [(410, LEAF), (last, CC)],                                           # shares word 12 with A; the last id of the last word
             CC: [(last, LEAF)],                                                     # shares the last word with B
             LEAF: [],
             LOOP: [(500, LOOP), (501, LEAF)]}                                       # an edge to itself
    flags = {ROOT: 2, A: 0, B: 1, CC: 0, LEAF: 1, LOOP: 0}
    off, tok, nxt = [0], [], []
    for s in range(6):
        for t, n in edges[s]:
            tok.append(t); nxt.append(n)
        off.append(len(tok))
    return LexiconTables(np.asarray(off, np.int32), np.asarray(tok, np.int32), np.asarray(nxt, np.int32),
                         np.asarray([flags[s] for s in range(6)], np.uint8), [ROOT], [{}], V, EOS, PAD, NOP)


def _case(lt, rows):
    """Per row: its slot, the slot's state and the token its head chose."""
    rng = np.random.default_rng(rows)
    S = rows + 3
    slots = rng.permutation(S)[:rows].astype(np.int32)
    state0, token = np.full(S, FREE_STATE, np.int32), np.full(S, -9, np.int32)
    last = lt.vocab - 1
    kinds = [(ROOT, lambda r: 300 + (r * 7) % 300), (A, lambda r: 400 + r % 26), (B, lambda r: last), (B, lambda r: EOS), (-1, lambda r: 410),
             (A, lambda r: NO_COLUMN), (B, lambda r: 410), (CC, lambda r: PAD), (ROOT, lambda r: NOP), (CC, lambda r: last),
             (LOOP, lambda r: 500), (LOOP, lambda r: 501)]               # the edge to itself, and the way out of that state
    for r in range(rows):
        st, t = kinds[r % len(kinds)]
        state0[slots[r]], token[slots[r]] = st, t(r)
    return S, slots, state0, token


@pytest.mark.parametrize("rows", [1, 64, 320])
@pytest.mark.parametrize("V", [1024, 81920])
def test_start_and_step_rewrite_the_slot_rows_as_the_host_does(hip_lib, V, rows):
    lt = _automaton(V)
    words = (V + 31) // 32
    S, slots, state0, token = _case(lt, rows)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = [torch.from_numpy(x).cuda() for x in (lt.edge_off, lt.edge_tok, lt.edge_next, lt.state_flags)]
    table = torch.full((ROW_BASE + S, words), -1, dtype=torch.int32, device="cuda")                       # 0xff everywhere
    slot_state = torch.full((S,), FREE_STATE, dtype=torch.int32, device="cuda")
    slot_mask = torch.full((S,), MASK_SENT, dtype=torch.int32, device="cuda")
    a = L.RecLexiconArgsC()
    a.edge_off, a.edge_tok, a.edge_next, a.state_flags = (t.data_ptr() for t in dev)
    a.table, a.slot_state, a.slot_mask = table.data_ptr(), slot_state.data_ptr(), slot_mask.data_ptr()
    a.words, a.row_base, a.vocab, a.eos_id, a.pad_id, a.nop_id = words, ROW_BASE, V, EOS, PAD, NOP

    def read():
        torch.cuda.synchronize()
        return table.cpu().numpy().view(np.uint32), slot_state.cpu().numpy(), slot_mask.cpu().numpy()

    # ---- start: the named slots take their states; a state >= 0 rewrites the whole row and names it
    d_slots, d_states = torch.from_numpy(slots).cuda(), torch.from_numpy(state0[slots]).cuda()
    assert hip_lib.surya_op_rec_lexicon_start(C.byref(a), d_slots.data_ptr(), d_states.data_ptr(), rows, stream) == 0
    tab, st, mk = read()
    want_tab = np.full((ROW_BASE + S, words), 0xffffffff, np.uint32)
    want_mask = np.full(S, MASK_SENT, np.int32)
    for s in slots:
        if state0[s] >= 0:
            want_tab[ROW_BASE + s], want_mask[s] = lt.row(int(state0[s])), ROW_BASE + s
    assert np.array_equal(st, state0), (st.tolist(), state0.tolist())
    assert np.array_equal(mk, want_mask)
    assert np.array_equal(tab, want_tab), np.argwhere(tab != want_tab)[:8].tolist()

    # ---- step: every row's slot moves behind its token, or touches nothing
    d_tok = torch.from_numpy(token).cuda()
    assert hip_lib.surya_op_rec_lexicon_step(C.byref(a), d_slots.data_ptr(), d_tok.data_ptr(), rows, stream) == 0
    tab, st, mk = read()
    state1 = state0.copy()
    moved = 0
    for s in slots:
        ns = lt.advance(int(state0[s]), int(token[s]))
        if ns != state0[s]:
            state1[s], want_tab[ROW_BASE + s] = ns, lt.row(ns)
            moved += 1
    assert moved >= max(1, rows // 2)
    assert np.array_equal(st, state1), (st.tolist(), state1.tolist())
    assert np.array_equal(mk, want_mask)                                           # a step never changes a mask id
    assert np.array_equal(tab, want_tab), np.argwhere(tab != want_tab)[:8].tolist()

    # ---- a second step over the same tokens: the slots that can move again do, the rest keep everything
    assert hip_lib.surya_op_rec_lexicon_step(C.byref(a), d_slots.data_ptr(), d_tok.data_ptr(), rows, stream) == 0
    tab, st, mk = read()
    state2 = state1.copy()
    for s in slots:
        ns = lt.advance(int(state1[s]), int(token[s]))
        if ns != state1[s]:
            state2[s], want_tab[ROW_BASE + s] = ns, lt.row(ns)
    assert np.array_equal(st, state2) and np.array_equal(mk, want_mask)
    assert np.array_equal(tab, want_tab), np.argwhere(tab != want_tab)[:8].tolist()


def test_the_hand_made_automaton_holds_the_cases():
    """(no GPU work) what the docstring promises about the automaton, checked on the host restatement."""
    lt = _automaton(81920)
    assert len(lt.edges(ROOT)[0]) == 300 > L_STEP_LANES
    assert {t >> 5 for t in lt.edges(A)[0].tolist()} == {12, 13}
    assert {t >> 5 for t in lt.allowed(A)} & {t >> 5 for t in lt.allowed(B)}          # an old and a new set share a word
    assert lt.accepts(LEAF) and len(lt.edges(LEAF)[0]) == 0
    assert max(lt.allowed(B)) == 81919 and 81919 >> 5 == 2559
    assert lt.advance(ROOT, NOP) == ROOT and NOP in lt.allowed(ROOT)
    assert lt.advance(LOOP, 500) == LOOP and lt.advance(LOOP, 501) == LEAF


L_STEP_LANES = 64       # SA_LEXICON_STEP_THREADS (csrc/lexicon.h)


def test_op_hooks_refuse_incomplete_operands(hip_lib):
    x = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p, s = x.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = L.RecLexiconArgsC()
    a.edge_off = a.edge_tok = a.edge_next = a.state_flags = a.table = a.slot_state = p       # slot_mask missing
    a.words, a.row_base, a.vocab = 4, 0, 128
    assert hip_lib.surya_op_rec_lexicon_start(C.byref(a), p, p, 1, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_lexicon_step(C.byref(a), p, p, 1, s) == L.SA_ERR_ARG
    a.slot_mask = p
    a.vocab = 129                                                                    # wider than the rows
    assert hip_lib.surya_op_rec_lexicon_step(C.byref(a), p, p, 1, s) == L.SA_ERR_ARG
    a.vocab = 128
    assert hip_lib.surya_op_rec_lexicon_start(C.byref(a), None, p, 1, s) == L.SA_ERR_ARG
    assert hip_lib.surya_op_rec_lexicon_step(C.byref(a), p, p, 0, s) == 0            # no rows: nothing to launch
    torch.cuda.synchronize()
