"""Decode-step A/B sweep inside ONE process (one gpurun call): REC-FULL bf16, 256 active slots, bench-shaped prompts.

For every tuning configuration (surya_set_tuning, csrc/common.h sa::Tuning) this re-prefills the same 256 lines, runs
`--steps` decode steps in calls of 4 (the predictor's steps_per_sync) with the next call enqueued before the previous one is
read, and reports wall us/step (HIP events around the whole run) plus whether the greedy tokens equal the first
configuration's (tile / split-K changes re-order fp32 sums, so bf16 argmax near-ties may flip; reported, not asserted).

    python tools/microbench/decode_sweep.py [--steps 32] [--configs all|base|fp8|mxbigm|masks|alts|forced|patterns|lexicon|boost] [--fp8] [--slots N]

`fp8`: bf16 decode vs the MXFP8 decode path (HipRecModel.set_decode_fp8, csrc/gemm_mx.h) on the same lines.
`--fp8`: every arm runs with set_decode_fp8(True) unless it says fp8=0 itself.
`mxbigm` (with --fp8 --slots 512 / 1024): the MXFP8 tiles above 256 rows (mx_big_m_split x mx_big_m_gateup), arm 0 = everything
64 x 64 run twice, the default twice, and the bf16 default of the same build as the last arm. Tokens are compared with the first
arm of the same arithmetic (fp8 with fp8, bf16 with bf16).

`masks`: the unmasked step against the step with a token mask on EVERY slot (HipRecModel.set_token_masks: the masked lm_head
epilogues), arms alternating none / digits allowlist / none / random 50 % mask / none. Tokens are compared with the first arm of the
same mask. `maskonly`: the digits arm alone.

`alts`: alternatives (HipRecModel.set_alternatives: the *_TOPK lm_head epilogue and the combine kernel behind the head) off / on / off /
on / off, alternating; tokens must be identical to the first arm. `altsonly`: the "on" arm alone (for a kernel trace beside `base`).

`forced`: forced decoding (HipRecModel.set_forced: the *_FORCED lm_head epilogue and the forced greedy head) off / on / off / on / off,
alternating, every slot forced to random ids for the whole run; the off arms' tokens must be identical to the first arm, the on arms emit
their ids. `forcedonly`: the "on" arm alone (for a kernel trace beside `base`).

`patterns`: pattern-guided decoding (HipRecModel.set_patterns: the greedy head advances every slot's automaton and mask id), three arms
alternating in one process: unmasked / masks only (digits allowlist) / a pattern on every slot, twice, then unmasked once more. pat=1 is
the date \d{2}/\d{2}/\d{4} (a line is complete after 10 tokens and keeps its state from then on), pat=2 is \d{64}, which takes a
transition at every step of the run. Tokens are compared with the first arm of the same constraint. `patternonly`: the date arm alone
(for a kernel trace beside `base` and `maskonly`).

`lexicon`: lexicon-guided decoding (HipRecModel.set_lexicon: lexicon_step_kernel behind every head rewrites each slot's own mask row),
arms alternating in one process: unmasked / masks only / the date pattern / a lexicon on every slot, twice, then unmasked once more --
three identical unmasked arms, whose spread is the noise band. lex=1 is 2000 random five-digit codes (a line is complete after 6 tokens
and keeps its state and row from then on), lex=2 is 300 entries with 300 different first characters and 40 digits each: a root with 300
children, and a transition at every step of the run. `lexicononly` / `lexiconwide`: the lex=1 / lex=2 arm alone (for a kernel trace).

`boost`: boosted decoding (HipRecModel.set_boost: a second, unmasked lm_head launch, boost_head_kernel in place of the greedy head and
boost_step_kernel behind it), arms alternating in one process: unmasked / masks only / boost on every slot, twice, then unmasked once
more -- three identical unmasked arms, whose spread is the noise band. bst=1 is 2000 random lower-case words of 5 to 9 letters at beta =
8 (on random weights most slots sit in the state without edges and rewrite nothing); bst=2 is 300 two-unit entries with 300 different
first characters and a full stop at beta = 1e4: every slot alternates between the root's 300-bit set and a one-bit set, a row rewrite at
every step. `boostonly` / `boostwide`: the bst=1 / bst=2 arm alone (for a kernel trace).

The tile-shape / dual-stream / lm_head-ring / skinny-GEMM variants swept in round 2 lost and were removed from the library; their
results are in profiles/r02_decode_sweeps.md.
"""
from __future__ import annotations

import argparse
import ctypes as C
import itertools
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--configs", default="all")
    ap.add_argument("--fp8", action="store_true", help="run every arm on the MXFP8 decode path (set_decode_fp8(True))")
    args = ap.parse_args()
    from surya_amd import _lib as L
    from surya_amd.config import rec_config
    from surya_amd.recognition.model import HipRecModel
    from surya_amd.synth import make_rec_weights
    from util import make_prompts, crop_grid

    lib = L.lib()
    cfg = rec_config("REC-FULL")
    sd = make_rec_weights(cfg, 0)
    n = args.slots
    m = HipRecModel(cfg, sd, image_token_id=cfg.image_token_id, pad_token_id=cfg.pad_token_id, eos_token_id=cfg.eos_token_id,
                    dtype=torch.bfloat16, max_slots=n, max_kv_len=64 + args.steps + 40, max_patches=65536, max_prefill_tokens=n * 72)
    rng = np.random.default_rng(1234)
    grids = [crop_grid(64, int(w)) for w in sorted(rng.integers(128, 513, size=n), reverse=True)]
    tiles, seqs = make_prompts(cfg, grids, seed=3)
    tiles = tiles.cuda().contiguous()
    slots = list(range(n))

    def setk(**kw):
        for k, v in kw.items():
            L.check(lib.surya_set_tuning(k.encode(), C.c_int(v)), f"surya_set_tuning({k})")

    base = dict(graph=0, split_target=256, split_min_kt=4, split_max=8, dattn=4, rnorm=2, ghead=2, fuse_embed=1, lmhead=1, kvprefetch=0, gateup_ring=2, big_m_split=-1, big_m_gateup=-1,
                mx_big_m_split=-1, mx_big_m_gateup=-1)
    if args.configs == "base":
        variants = [dict()]
    elif args.configs == "fewer":        # fewer, longer split-K slices for the bf16 path
        variants = [dict(), dict(split_min_kt=6), dict(split_min_kt=8), dict(split_min_kt=10), dict(split_max=2), dict(split_target=192),
                    dict(split_target=128), dict(split_max=1)]
    elif args.configs == "r4":           # round 4: every new decode-step kernel against the round-3 kernel it replaces, one at a time
        variants = [dict(), dict(dattn=3), dict(rnorm=1), dict(ghead=1, fuse_embed=0), dict(fuse_embed=0), dict(lmhead=0), dict(lmhead=2),
                    dict(dattn=3, rnorm=1, ghead=1, fuse_embed=0, lmhead=0), dict(graph=1), dict()]
    elif args.configs == "r5":           # round 5: LDS stages of the decode gate|up loop (2 = unrolled pair, 3 / 4 = ring with counted vmcnt), interleaved
        variants = [dict(), dict(gateup_ring=3), dict(gateup_ring=4), dict(), dict(gateup_ring=3), dict(gateup_ring=4)]
    elif args.configs == "bigm":         # round 6: tiles of the decode projections above 256 rows (run with --slots 512 / 1024), interleaved
        variants = [dict(big_m_split=0, big_m_gateup=0), dict(), dict(big_m_split=2, big_m_gateup=0), dict(big_m_split=3, big_m_gateup=0),
                    dict(big_m_split=0, big_m_gateup=2), dict(big_m_split=2, big_m_gateup=2), dict(big_m_split=2, big_m_gateup=1),
                    dict(big_m_split=0, big_m_gateup=0), dict()]
    elif args.configs == "mxbigm":       # round 10: MXFP8 tiles above 256 rows (run with --fp8 --slots 512 / 1024), arm 0 and the default twice, bf16 last
        variants = [dict(mx_big_m_split=0, mx_big_m_gateup=0), dict()]
        variants += [dict(mx_big_m_split=sp, mx_big_m_gateup=gu) for gu in (0, 1, 2) for sp in (0, 2, 3) if (sp, gu) != (0, 0)]
        variants += [dict(mx_big_m_split=0, mx_big_m_gateup=0), dict(), dict(fp8=0)]
    elif args.configs == "masks":        # constrained output: a mask on every slot against none, alternating
        variants = [dict(), dict(masks=1), dict(), dict(masks=2), dict()]
    elif args.configs == "maskonly":     # one arm, a digits allowlist on every slot (for a kernel trace beside `base`)
        variants = [dict(masks=1)]
    elif args.configs == "patterns":     # pattern-guided decoding: unmasked / masks only / a pattern on every slot, alternating
        variants = [dict(), dict(masks=1), dict(pat=1), dict(pat=2), dict(), dict(masks=1), dict(pat=1), dict(pat=2), dict()]
    elif args.configs == "patternonly":  # one arm, the date pattern on every slot (for a kernel trace beside `base` / `maskonly`)
        variants = [dict(pat=1)]
    elif args.configs == "lexicon":      # lexicon-guided decoding against unmasked / masks only / the date pattern, alternating
        arms = [dict(), dict(masks=1), dict(pat=1), dict(lex=1), dict(lex=2)]
        variants = arms + arms + [dict()]
    elif args.configs in ("lexicononly", "lexiconwide"):     # one arm, a lexicon on every slot (for a kernel trace)
        variants = [dict(lex=1 if args.configs == "lexicononly" else 2)]
    elif args.configs == "boost":        # boosted decoding against unmasked / masks only, alternating
        arms = [dict(), dict(masks=1), dict(bst=1), dict(bst=2)]
        variants = arms + arms + [dict()]
    elif args.configs in ("boostonly", "boostwide"):         # one arm, boosting on every slot (for a kernel trace)
        variants = [dict(bst=1 if args.configs == "boostonly" else 2)]
    elif args.configs == "alts":         # alternatives: off against on, alternating
        variants = [dict(), dict(alts=1), dict(), dict(alts=1), dict()]
    elif args.configs == "altsonly":
        variants = [dict(alts=1)]
    elif args.configs == "forced":       # forced decoding: off against on, alternating
        variants = [dict(), dict(forced=1), dict(), dict(forced=1), dict()]
    elif args.configs == "forcedonly":
        variants = [dict(forced=1)]
    elif args.configs == "pf":           # K/V prefetch workgroups in the reduce kernels, on / off, interleaved
        variants = [dict(kvprefetch=1), dict(), dict(kvprefetch=1), dict(), dict(lmhead=2, kvprefetch=1), dict(lmhead=2)]
    elif args.configs == "fp8only":
        variants = [dict(fp8=1)]
    elif args.configs == "fp8":
        variants = [dict(), dict(fp8=1), dict(fp8=1, split_min_kt=2), dict(fp8=1, split_min_kt=3), dict(fp8=1, split_target=320)]
    else:
        variants = [dict(), dict(graph=1), dict(split_target=512), dict(split_target=384), dict(split_target=192), dict(split_min_kt=2),
                    dict(split_max=4)]

    stop_ids = (cfg.eos_token_id, cfg.pad_token_id)
    forced_ids = [[int(t) if t not in stop_ids else 17 for t in row]
                  for row in np.random.default_rng(99).integers(0, cfg.decoder.vocab_size, size=(n, args.steps + 1))]

    pat_start = [None]
    lex_start = [None]
    bst_start = [None]                               # (root, beta)

    def run(n_steps):
        if bst_start[0] is not None:                 # every run starts every slot at its root again
            m.set_slot_masks(slots, [-1] * n)
            m.set_slot_boost(slots, [bst_start[0][0]] * n, bst_start[0][1])
        if lex_start[0] is not None:                 # every run starts every slot's lexicon again
            m.set_slot_masks(slots, [-1] * n)
            m.set_slot_lexicon(slots, [lex_start[0]] * n)
        if pat_start[0] is not None:                 # every run starts every slot's automaton again
            m.set_slot_masks(slots, [-1] * n)
            m.set_slot_patterns(slots, [pat_start[0]] * n)
        if m.forced:
            m.set_forced_tokens(slots, [row[: n_steps + 1] for row in forced_ids])
        m.prefill(tiles, grids, seqs, slots)
        m.read_outputs(1)
        m.set_active(slots)
        toks = []
        calls = [(min(4, n_steps - i), (i // 4) & 1) for i in range(0, n_steps, 4)]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        m.decode_async(*calls[0])
        for i, call in enumerate(calls):
            if i + 1 < len(calls):
                m.decode_async(*calls[i + 1])
            t, _, _ = m.wait_outputs(*call)
            if m.alternatives:
                m.wait_alternatives(*call)               # what the device loop reads beside the tokens
            if m.forced:
                m.wait_forced(*call)
            if m.n_boost_states:
                m.wait_boost(*call)
            toks.append(t[: call[0], :n].copy())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n_steps, (time.perf_counter() - t0) * 1e6 / n_steps, np.concatenate(toks)

    def set_masks(kind):                         # 0 = off, 1 = digits allowlist, 2 = a random half of the vocabulary (+ the control ids)
        if not kind:
            return m.set_token_masks(None)
        from surya_amd.recognition.loader import RecognitionModelLoader
        tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
        V = cfg.decoder.vocab_size
        mask = tk.token_mask(allow="0123456789.,-", vocab_size=V)
        if kind == 2:
            mask = mask | np.random.default_rng(7).integers(0, 2 ** 32, size=mask.shape, dtype=np.uint32)
            mask[-1] &= np.uint32((1 << (V - 32 * (len(mask) - 1))) - 1) if V % 32 else np.uint32(0xFFFFFFFF)
        m.set_token_masks(mask[None])
        m.set_slot_masks(slots, [0] * n)

    def set_patterns(kind):                      # 0 = off (the mask table goes too), 1 = the date, 2 = 64 digits: a transition at every step
        pat_start[0] = None
        if not kind:
            return m.set_token_masks(None)
        from surya_amd.recognition.loader import RecognitionModelLoader
        from surya_amd.recognition.pattern import compile_patterns
        tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
        pt = compile_patterns(tk, [r"\d{2}/\d{2}/\d{4}" if kind == 1 else r"\d{64}"], cfg.decoder.vocab_size)
        m.set_token_masks(pt.table.array())
        m.set_patterns(pt)
        pat_start[0] = pt.starts[0]

    def set_lexicon(kind):                       # 0 = off (the mask table goes too), 1 = 2000 five-digit codes, 2 = a root with 300 children
        lex_start[0] = pat_start[0] = None
        if not kind:
            return m.set_token_masks(None)
        import random
        from surya_amd.recognition.lexicon import compile_lexicons
        from surya_amd.recognition.loader import RecognitionModelLoader
        tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
        r = random.Random(2)
        entries = (["%05d" % r.randrange(100000) for _ in range(2000)] if kind == 1 else
                   [chr(0x100 + k) + "".join(r.choice("0123456789") for _ in range(40)) for k in range(300)])
        lt = compile_lexicons(tk, [entries], cfg.decoder.vocab_size)
        m.set_token_masks(tk.token_mask(allow="0123456789.,-", vocab_size=cfg.decoder.vocab_size)[None])     # (a lexicon needs a mask table)
        m.set_lexicon(lt)
        lex_start[0] = lt.starts[0]

    def set_boost(kind):                         # 0 = off (the mask table goes too), 1 = 2000 words at beta 8, 2 = a root with 300 children at 1e4
        bst_start[0] = None
        if not kind:
            return m.set_token_masks(None)
        import random
        from surya_amd.recognition.boost import compile_boost
        from surya_amd.recognition.loader import RecognitionModelLoader
        tk = RecognitionModelLoader({"config": cfg, "state_dict": {}}).processor().ocr_tokenizer
        r = random.Random(2)
        entries = (["".join(r.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(5, 9))) for _ in range(2000)] if kind == 1 else
                   [chr(0x100 + k) + "." for k in range(300)])
        bt = compile_boost(tk, [entries], cfg.decoder.vocab_size)
        bt.word_row = 0
        m.set_token_masks(bt.word_mask[None])        # (boosting needs a mask table: the word-unit row)
        m.set_boost(bt)
        bst_start[0] = (bt.roots[0], 8.0 if kind == 1 else 1e4)

    lex_cfg = args.configs in ("lexicon", "lexicononly", "lexiconwide")
    bst_cfg = args.configs in ("boost", "boostonly", "boostwide")
    ref = {}
    print(f"# REC-FULL bf16, {n} active slots, {args.steps} decode steps per run, us/step (event) | us/step (host wall) | tokens == first arm of the same arithmetic")
    for v in variants:
        v = dict(v)
        m.set_decode_fp8(bool(v.pop("fp8", int(args.fp8))))
        masks = v.pop("masks", 0)
        alts = v.pop("alts", 0)
        if alts or args.configs in ("alts", "altsonly"):
            m.set_alternatives(bool(alts))
        forced = v.pop("forced", 0)
        if forced or args.configs in ("forced", "forcedonly"):
            m.set_forced(bool(forced))
        pat = v.pop("pat", 0)
        lex = v.pop("lex", 0)
        if lex_cfg:
            set_lexicon(lex)                         # (off: the mask table and patterns go too; the arm's own constraint follows)
        bst = v.pop("bst", 0)
        if bst_cfg:
            set_boost(bst)                           # (likewise)
            if masks:
                set_masks(masks)
        if pat:
            set_patterns(pat)
        elif args.configs in ("patterns", "patternonly"):
            set_patterns(0)
            if masks:
                set_masks(masks)
        if (masks and not bst_cfg) or args.configs in ("masks", "maskonly"):
            set_masks(masks)
        setk(**{**base, **v})
        v = {**v, "fp8": int(m.decode_fp8)}
        if args.configs in ("masks", "maskonly", "patterns", "patternonly") or lex_cfg:
            v["masks"] = masks
            if args.configs in ("patterns", "patternonly") or lex_cfg:
                v["pat"] = pat
            if lex_cfg:
                v["lex"] = lex
        if bst_cfg:
            v.update(masks=masks, bst=bst)
        if args.configs in ("alts", "altsonly"):
            v["alts"] = alts
        if args.configs in ("forced", "forcedonly"):
            v["forced"] = forced
        run(8)                                   # warm-up (attribute set, graph capture on 2nd sight)
        run(8)
        best = min((run(args.steps) for _ in range(3)), key=lambda r: r[0])
        same = float((best[2] == ref.setdefault((v["fp8"], v.get("masks", 0), v.get("forced", 0), v.get("pat", 0), v.get("lex", 0), v.get("bst", 0)), best[2])).all(axis=0).mean())
        print(f"{str(v):90s} {best[0]:8.1f} {best[1]:8.1f}   lines identical {same:.3f}", flush=True)
    setk(**base)
    m.set_decode_fp8(False)
    if args.configs in ("masks", "maskonly", "patterns", "patternonly") or lex_cfg or bst_cfg:
        m.set_token_masks(None)                      # (which switches patterns, the lexicon and boosting off as well)
    if args.configs in ("alts", "altsonly"):
        m.set_alternatives(False)
    if args.configs in ("forced", "forcedonly"):
        m.set_forced(False)


if __name__ == "__main__":
    main()
