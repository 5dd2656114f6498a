"""GPU: beam search's two kernels alone, through the launchers the engine uses (surya_op_rec_beam_select / surya_op_rec_kv_fork).

beam_select_kernel against csrc/beam_core.h compiled for the host (tests/beam_ref.py; tests/test_beam_cpu.py checks that build against the
rules in Python): every output equal, the scores bit for bit. kv_fork_kernel against a numpy copy of the same ranges: the WHOLE cache
afterwards equals the expectation byte for byte, so nothing outside the ranges moved."""
import ctypes as C

import numpy as np
import pytest
import torch

from surya_amd import _lib as L

import beam_ref as br

pytestmark = pytest.mark.gpu
EOS, PAD, NOP = 1, 0, 3
DT = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("first", [False, True])
def test_beam_select_equals_the_host_build_of_the_core(hip_lib, B, first):
    """40 random groups (ties, frozen and empty beams, short rows, one parent ahead) behind a shuffled lead-slot list, 3 unused slots at the end."""
    rng = np.random.default_rng(10 * B + first)
    G = 40
    n = G * B + 3
    score, fin, ids, ps = br.random_groups(rng, G, B, EOS, PAD, NOP, first)
    want = br.native_select(G, B, score, fin, ids, ps, EOS, PAD, NOP, first)
    pad3 = lambda a, v: np.concatenate([a, np.full((3,) + a.shape[1:], v, a.dtype)])
    d_score, d_fin, d_ids, d_ps = _dev(pad3(score, 7)), _dev(pad3(fin, 7)), _dev(pad3(ids, 7)), _dev(pad3(ps, 7))
    lead = rng.permutation(G).astype(np.int32) * B               # groups in any order: one wave each, no wave touches another group
    stride = 2
    lead_list = np.full(G * stride, -99, np.int32)
    lead_list[::stride] = lead
    out_i = {k: torch.full((n,), -77, dtype=torch.int32, device="cuda") for k in ("token", "parent", "rank", "next", "fork_src")}
    out_f = {k: torch.full((n,), -77.0, dtype=torch.float32, device="cuda") for k in ("prob", "logp")}
    kv_len = rng.integers(5, 50, size=n).astype(np.int32)
    prompt = rng.integers(1, 5, size=n).astype(np.int32)
    d_kv, d_prompt = _dev(kv_len), _dev(prompt)
    d_base, d_len = torch.full((n,), -77, dtype=torch.int32, device="cuda"), torch.full((n,), -77, dtype=torch.int32, device="cuda")
    Tmax = 40
    d_lead = _dev(lead_list)
    rc = L.lib().surya_op_rec_beam_select(L.ptr(d_lead), stride, G, B, n, L.ptr(d_ids), L.ptr(d_ps), L.ptr(d_score), L.ptr(d_fin), EOS, PAD, NOP,
                                          int(first), L.ptr(out_i["token"]), L.ptr(out_i["parent"]), L.ptr(out_i["rank"]), L.ptr(out_f["prob"]),
                                          L.ptr(out_f["logp"]), L.ptr(out_i["next"]), L.ptr(out_i["fork_src"]), L.ptr(d_kv), L.ptr(d_prompt),
                                          L.ptr(d_base), L.ptr(d_len), Tmax, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    m = G * B
    for k in ("token", "parent", "rank", "fork_src"):
        assert np.array_equal(out_i[k].cpu().numpy()[:m], want[k]), k
    assert out_f["logp"].cpu().numpy()[:m].tobytes() == want["logp"].tobytes(), "scores differ in some bit from float32(cum + log p)"
    assert out_f["prob"].cpu().numpy()[:m].tobytes() == want["prob"].tobytes()
    assert np.array_equal(d_fin.cpu().numpy()[:m], want["finished"]) and d_score.cpu().numpy()[:m].tobytes() == want["logp"].tobytes()
    assert np.array_equal(out_i["next"].cpu().numpy()[:m], np.where(want["finished"] == 1, PAD, want["token"]))
    # the engine's slot state: lengths and the fork plan
    lead_of = (np.arange(m) // B) * B
    was_empty = np.ones(m, bool) if first else (fin == 1) & np.isneginf(score)
    want_prompt = kv_len[lead_of] if first else prompt[:m]
    assert np.array_equal(d_kv.cpu().numpy()[:m], kv_len[lead_of] if first else kv_len[:m])
    assert np.array_equal(d_prompt.cpu().numpy()[:m], want_prompt)
    assert np.array_equal(d_base.cpu().numpy()[:m], np.where(was_empty, 0, want_prompt))
    assert np.array_equal(d_len.cpu().numpy()[:m], np.minimum(kv_len[lead_of], Tmax))
    # the three slots no group owns: untouched
    for t in list(out_i.values()) + list(out_f.values()) + [d_base, d_len]:
        assert (t.cpu().numpy()[m:] == -77).all()
    assert np.array_equal(d_kv.cpu().numpy()[m:], kv_len[m:]) and (d_fin.cpu().numpy()[m:] == 7).all()


def test_beam_select_refuses_bad_arguments(hip_lib):
    z = torch.zeros(16, dtype=torch.int32, device="cuda")
    f = torch.zeros(16, dtype=torch.float32, device="cuda")
    call = lambda width, n_slots, tok: L.lib().surya_op_rec_beam_select(None, 1, 1, width, n_slots, L.ptr(z), L.ptr(f), L.ptr(f), L.ptr(z), EOS, PAD, NOP,
                                                                       0, tok, L.ptr(z), L.ptr(z), L.ptr(f), L.ptr(f), L.ptr(z), L.ptr(z), None, None,
                                                                       None, None, 0, _stream())
    assert call(1, 4, L.ptr(z)) == L.SA_ERR_ARG and call(5, 8, L.ptr(z)) == L.SA_ERR_ARG      # widths outside 2..4
    assert call(4, 3, L.ptr(z)) == L.SA_ERR_ARG                                                # the group does not fit the slots
    assert call(2, 4, None) == L.SA_ERR_ARG
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [32, 128])
def test_kv_fork_copies_exactly_the_ranges(hip_lib, dtype, D):
    """2 layers, 8 slots, 2 kv heads, max_kv_len 40; range lengths 0, 1, 7 and 33, two destinations sharing a source, some slots without a
    fork, one base below 0 and one len above max_kv_len (clamped)."""
    layers, S, nkv, Tmax = 2, 8, 2, 40
    g = torch.Generator().manual_seed(D)
    k = torch.randn((layers, S, nkv, Tmax, D), generator=g).to(dtype).cuda()
    v = torch.randn((layers, S, nkv, Tmax, D), generator=g).to(dtype).cuda()
    #          slot:  0   1   2   3   4   5   6   7
    src = np.array([-1,  0,  0, -1,  3, -1,  3,  5], np.int32)         # 1 and 2 share source 0; 4 and 6 share source 3
    base = np.array([0,  3,  5,  0,  7, 0, -2, 39], np.int32)
    ln = np.array([40, 36,  6, 40,  7, 9,  7, 45], np.int32)           # lengths 33, 1, -, 0, -, 7 (clamped base), 1 (clamped len)
    as_bytes = lambda t: t.cpu().contiguous().view(torch.uint8).numpy().copy()
    want_k, want_v = as_bytes(k), as_bytes(v)
    for want in (want_k, want_v):
        w = want.reshape(layers, S, nkv, Tmax, -1)
        orig = w.copy()
        for d in range(S):
            if src[d] >= 0:
                a, b = max(int(base[d]), 0), min(int(ln[d]), Tmax)
                w[:, d, :, a:b] = orig[:, src[d], :, a:b]
    assert sorted(min(l, Tmax) - max(b, 0) for s, b, l in zip(src, base, ln) if s >= 0) == [0, 1, 1, 7, 33]
    d_src, d_base, d_ln = _dev(src), _dev(base), _dev(ln)          # (named: a temporary's memory would be handed to the next one)
    rc = L.lib().surya_op_rec_kv_fork(DT[dtype], L.ptr(k), L.ptr(v), L.ptr(d_src), L.ptr(d_base), L.ptr(d_ln), S, layers, S, nkv, Tmax, D, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert as_bytes(k).tobytes() == want_k.tobytes() and as_bytes(v).tobytes() == want_v.tobytes()
    assert not np.array_equal(want_k, as_bytes(torch.randn((layers, S, nkv, Tmax, D), generator=torch.Generator().manual_seed(D)).to(dtype)))


def test_kv_fork_refusals(hip_lib):
    k = torch.zeros(2 * 4 * 2 * 8 * 32, dtype=torch.float16, device="cuda")
    i = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    call = lambda dt, D, rows: L.lib().surya_op_rec_kv_fork(dt, L.ptr(k), L.ptr(k), L.ptr(i), L.ptr(i), L.ptr(i), rows, 2, 4, 2, 8, D, _stream())
    assert call(7, 32, 4) == L.SA_ERR_UNSUPPORTED                  # an unknown dtype
    assert call(L.DTYPE_F16, 4, 4) == L.SA_ERR_SHAPE               # rows of 8 bytes: no 16-byte units
    assert call(L.DTYPE_F16, 32, 5) == L.SA_ERR_ARG                # more rows than slots
    assert call(L.DTYPE_F16, 32, 4) == 0                           # every fork_src -1: nothing to do
    torch.cuda.synchronize()
