"""HipDetModel: the detection forward pass behind libsurya_amd.so (no CPU fallback)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..config import DetConfig
from .plan import build_det_plan


class DetOpC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("type", "in0", "in1", "out", "res", "cin", "cout", "k", "stride", "act", "hin", "win",
                                         "hout", "wout", "w_idx", "b_idx", "p0", "p1")]


# compute dtypes of the engine: fp32 = reference mode; bf16 = the default; fp16 = the reference's GPU default (surya settings.MODEL_DTYPE)
_DTYPES = {torch.float32: L.DTYPE_F32, torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}


class HipDetModel:
    def __init__(self, cfg: DetConfig, state_dict, *, height: int, width: int, dtype: torch.dtype = torch.bfloat16,
                 device="cuda:0", max_batch: int = 16, broadcast_weights: bool = False, process_group=None):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetModel needs a GPU (MI355X); there is no CPU fallback")
        if dtype not in _DTYPES:
            raise ValueError("dtype must be float32 (reference mode), bfloat16 or float16")
        self.lib = L.lib()
        self.lib.surya_det_create.argtypes = None
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.height, self.width, self.max_batch = height, width, max_batch
        torch.cuda.set_device(self.device)
        plan = build_det_plan(cfg, state_dict, height, width)
        # algorithmic FLOPs per page = the reference's own op order; the folded decode head executes fewer
        self.flops_per_image = plan.reference_flops_per_image
        self.executed_flops_per_image = plan.flops_per_image
        self.in_shape = (cfg.num_channels, height, width)
        self.num_labels = cfg.num_labels
        self._create(plan, broadcast_weights, process_group)

    @classmethod
    def from_plan(cls, plan, *, height: int, width: int, num_labels: int, dtype: torch.dtype = torch.bfloat16, max_batch: int = 16,
                  device="cuda:0"):
        """Test and measurement support: an engine over `plan` (a DetPlan) as it stands -- no config, no state dict. height / width /
        num_labels size the fp32 planes and the heat maps (surya_det_config); the pixels `forward` takes are those of the plan's INPUT op."""
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetModel needs a GPU (MI355X); there is no CPU fallback")
        if dtype not in _DTYPES:
            raise ValueError("dtype must be float32 (reference mode), bfloat16 or float16")
        from .plan import OP_INPUT
        self = cls.__new__(cls)
        self.lib = L.lib()
        self.lib.surya_det_create.argtypes = None
        self.cfg, self.dtype, self.device = None, dtype, torch.device(device)
        self.height, self.width, self.max_batch, self.num_labels = height, width, max_batch, num_labels
        torch.cuda.set_device(self.device)
        self.flops_per_image = self.executed_flops_per_image = plan.flops_per_image
        inp = [o for o in plan.ops if o["type"] == OP_INPUT]
        self.in_shape = (inp[0]["cin"], inp[0]["hin"], inp[0]["win"]) if inp else (0, 0, 0)
        self._create(plan, False, None)
        return self

    def _create(self, plan, broadcast_weights, process_group):
        from .plan import OP_LITEMLA, OP_UPSUM_SRC
        dtype, height, width, max_batch = self.dtype, self.height, self.width, self.max_batch
        self.launches_per_forward = sum(2 if o["type"] == OP_LITEMLA else (0 if o["type"] == OP_UPSUM_SRC else 1) for o in plan.ops)
        self.plan_ops = [dict(o) for o in plan.ops]
        self.buf_elems = list(plan.buf_elems)
        self.weights = [w.to(device=self.device, dtype=dtype).contiguous() for w in plan.weights]
        if broadcast_weights:             # every rank planned the op list (shapes); the folded weights used are rank 0's
            from .. import dist as sdist
            if sdist.collectives_on(process_group):
                cdev = sdist.collective_device(self.device, process_group)
                tmp = [w.to(cdev) for w in self.weights]
                sdist.broadcast_tensors(tmp, src=0, group=process_group)
                for w, t in zip(self.weights, tmp):
                    w.copy_(t)
        ops = (DetOpC * len(plan.ops))(*[DetOpC(**{k: v for k, v in o.items() if k != "tag"}) for o in plan.ops])
        table = (C.c_void_p * max(1, len(self.weights)))(*[w.data_ptr() for w in self.weights])
        bufs = (C.c_size_t * len(plan.buf_elems))(*plan.buf_elems)
        c = L.DetConfigC(n_ops=len(plan.ops), max_batch=max_batch, height=height, width=width, num_labels=self.num_labels,
                         dtype=_DTYPES[dtype])
        self.handle = C.c_void_p()
        L.check(self.lib.surya_det_create(C.byref(c), ops, table, len(self.weights), bufs, len(plan.buf_elems),
                                          C.byref(self.handle)), "surya_det_create")

    def __del__(self):
        h = getattr(self, "handle", None)
        if h:
            self.lib.surya_det_destroy(h)
            self.handle = None

    @property
    def config(self):
        return self.cfg

    def to(self, device_dtype=None):
        """See HipRecModel.to: same-placement requests are no-ops, anything else needs a new handle."""
        if device_dtype is None or device_dtype == self.dtype:
            return self
        if not isinstance(device_dtype, torch.dtype) and torch.device("cuda:0" if device_dtype == "cuda" else device_dtype) == self.device:
            return self
        raise NotImplementedError(f"HipDetModel lives on {self.device} as {self.dtype}; create a new predictor for {device_dtype}")

    def eval(self):
        return self

    def forward(self, pixel_values: torch.Tensor, want_lowres: bool = False):
        """pixel_values cuda fp32 [B,3,H,W] -> heatmaps fp32 [B, labels, H, W] (and [B, labels, H/4, W/4])."""
        assert pixel_values.is_cuda and pixel_values.dtype == torch.float32 and pixel_values.is_contiguous()
        B = pixel_values.shape[0]
        assert tuple(pixel_values.shape[1:]) == self.in_shape and B <= self.max_batch
        torch.cuda.set_device(self.device)
        # (a plan without UPSAMPLE_OUT / CLASSIFY leaves these untouched: the ABI wants a non-null heat pointer all the same)
        heat = torch.empty((B, self.num_labels, self.height, self.width), dtype=torch.float32, device=self.device)
        low = torch.empty((B, self.num_labels, self.height // 4, self.width // 4), dtype=torch.float32,
                          device=self.device) if want_lowres else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_forward(self.handle, L.ptr(pixel_values), C.c_int(B), L.ptr(heat), L.ptr(low), stream),
                "surya_det_forward")
        return (heat, low) if want_lowres else heat

    def read_buffer(self, buf: int, batch: int, shape):
        """Test and measurement support (surya_det_read_buffer): the first `batch` images of activation buffer `buf` after a forward,
        as a tensor of the compute dtype shaped [batch, *shape] (NHWC: shape = (h, w, c) of the op that wrote it)."""
        n = 1
        for d in shape:
            n *= int(d)
        assert 0 <= buf < len(self.buf_elems) and n == self.buf_elems[buf], "shape must cover the whole buffer"
        torch.cuda.set_device(self.device)
        out = torch.empty((batch, *shape), dtype=self.dtype, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_read_buffer(self.handle, C.c_int(buf), C.c_int(batch), L.ptr(out), C.c_size_t(out.numel() * out.element_size()),
                                               stream), "surya_det_read_buffer")
        return out

    def forward_timed(self, pixel_values: torch.Tensor):
        """Measurement support (surya_det_forward_timed): the same forward with a hipEvent in front of every op of the plan.
        Returns (heat maps, [(op dict, ms)]); ops folded into a fused form (sa::Tuning det_fuse) report 0 ms."""
        assert pixel_values.is_cuda and pixel_values.dtype == torch.float32 and pixel_values.is_contiguous()
        B = pixel_values.shape[0]
        torch.cuda.set_device(self.device)
        heat = torch.empty((B, self.num_labels, self.height, self.width), dtype=torch.float32, device=self.device)
        n = int(self.lib.surya_det_op_count(self.handle))
        ms = (C.c_float * n)()
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_forward_timed(self.handle, L.ptr(pixel_values), C.c_int(B), L.ptr(heat), L.ptr(None), stream, ms, C.c_int(n)),
                "surya_det_forward_timed")
        return heat, list(zip(self.plan_ops, [float(v) for v in ms]))

    def forward_u8(self, pages_u8: torch.Tensor, mean, std, want_lowres: bool = False):
        """pages cuda uint8 [B, H, W, 3 | 4] (RGB or RGBX, already at the processor size) -> heat maps; rescale + normalise run
        on the device."""
        assert pages_u8.is_cuda and pages_u8.dtype == torch.uint8 and pages_u8.is_contiguous()
        B, pix = pages_u8.shape[0], pages_u8.shape[3]
        assert tuple(pages_u8.shape[1:3]) == (self.height, self.width) and pix in (3, 4) and B <= self.max_batch
        torch.cuda.set_device(self.device)
        heat = torch.empty((B, self.num_labels, self.height, self.width), dtype=torch.float32, device=self.device)
        low = torch.empty((B, self.num_labels, self.height // 4, self.width // 4), dtype=torch.float32,
                          device=self.device) if want_lowres else None
        m = (C.c_float * 3)(*[float(np.float32(v)) for v in mean])
        sd = (C.c_float * 3)(*[float(np.float32(v)) for v in std])
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_forward_u8(self.handle, L.ptr(pages_u8), C.c_int(pix), m, sd, C.c_int(B), L.ptr(heat), L.ptr(low), stream),
                "surya_det_forward_u8")
        return (heat, low) if want_lowres else heat


class HipDetPost:
    """Heat map -> boxes on the device (surya_det_boxes, csrc/det_post.h): thresholds, 4-connected labelling, per-component
    dilation + minimum-area rectangle and confidences for all pages of a batch in a handful of launches; only the corner
    arrays come back to the host. No CPU fallback: this IS detect_boxes of the product path (surya/detection/heatmap.py:27-107)."""

    def __init__(self, device="cuda:0", max_boxes: int = 4096):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetPost needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.lib()
        self.device = torch.device(device)
        self.max_boxes = max_boxes
        self._ws = None

    def _workspace(self, B, H, W):
        need = int(self.lib.surya_det_boxes_workspace_bytes(C.c_int(B), C.c_int(H), C.c_int(W), C.c_int(self.max_boxes)))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws, need

    def launch(self, heat: torch.Tensor, text_threshold: float, low_text: float):
        """Enqueue the post-processing of a batch of maps and the D2H of its (small, fixed-size) outputs into pinned memory;
        returns a handle for `collect`. Nothing here waits for the GPU, so a caller can prepare and launch the NEXT batch before
        it looks at this one (DetectionPredictor._detect_device does)."""
        assert heat.is_cuda and heat.dtype == torch.float32 and heat.is_contiguous()
        if heat.dim() == 4:
            B, Lb, H, W = heat.shape
            stride = Lb * H * W
        else:
            B, H, W = heat.shape
            stride = H * W
        torch.cuda.set_device(self.device)
        ws, need = self._workspace(B, H, W)
        boxes = torch.empty((B, self.max_boxes, 4, 2), dtype=torch.float32, device=self.device)
        conf = torch.empty((B, self.max_boxes), dtype=torch.float32, device=self.device)
        count = torch.empty((B,), dtype=torch.int32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_boxes(L.ptr(heat), C.c_long(stride), C.c_int(B), C.c_int(H), C.c_int(W), C.c_float(text_threshold),
                                         C.c_float(low_text), C.c_int(self.max_boxes), L.ptr(boxes), L.ptr(conf), L.ptr(count), L.ptr(ws),
                                         C.c_size_t(need), stream), "surya_det_boxes")
        # 148 KB per page: cheaper to copy whole than to wait for the counts first
        hb = torch.empty(boxes.shape, dtype=torch.float32, pin_memory=True).copy_(boxes, non_blocking=True)
        hc = torch.empty(conf.shape, dtype=torch.float32, pin_memory=True).copy_(conf, non_blocking=True)
        hn = torch.empty(count.shape, dtype=torch.int32, pin_memory=True).copy_(count, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return (ev, hb, hc, hn, heat, (text_threshold, low_text))     # `heat` rides along: its memory must outlive the kernels

    def collect(self, pending):
        ev, hb, hc, hn, heat, thr = pending
        ev.synchronize()
        n = hn.numpy()
        bh, ch = hb.numpy(), hc.numpy()
        out = [(bh[b, : n[b]].copy(), ch[b, : n[b]].copy()) if n[b] >= 0 else None for b in range(len(n))]
        over = [b for b in range(len(n)) if n[b] < 0]
        if over:
            # a noisy / very dense page: more kept components than the (fixed-size, copied-whole) output holds. The reference has
            # no cap, so run those pages again, alone, with room for 16 x as many boxes; only past that give up loudly.
            if self.max_boxes >= 1 << 16:
                self._raise_overflow()
            big = HipDetPost(self.device, max_boxes=self.max_boxes * 16)
            redo = big(heat[over].contiguous(), *thr)
            for b, r in zip(over, redo):
                out[b] = r
        return out

    def _raise_overflow(self):
        raise L.SuryaAmdError(f"surya_det_boxes: a page has more than max_boxes = {self.max_boxes} text components")

    def __call__(self, heat: torch.Tensor, text_threshold: float, low_text: float):
        """heat: cuda fp32, [B, H, W] contiguous, or a [B, labels, H, W] tensor whose plane 0 is the text map (then the page
        stride is labels * H * W). Returns a list of (boxes float32 [n, 4, 2], confidences float32 [n]) per page, in the
        component order cv2.connectedComponentsWithStats would label them."""
        return self.collect(self.launch(heat, text_threshold, low_text))


class HipDetSkew:
    """Heat map -> projection-profile scores of every candidate angle on the device (surya_det_skew, csrc/det_skew.h): the estimator
    behind DetectionPredictor.skew (detection/skew.py states the rule and chooses the angle from the scores). Owns the workspace; `launch`
    enqueues behind whatever is on the stream (the predictor: behind surya_det_boxes of the same maps), `collect` waits for ITS event."""

    def __init__(self, device="cuda:0"):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetSkew needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.bind_det_skew(L.lib())
        self.device = torch.device(device)
        self._ws = None

    def _workspace(self, B, H, W):
        need = int(self.lib.surya_det_skew_workspace_bytes(B, H, W))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws, need

    def launch(self, heat: torch.Tensor, tables: np.ndarray, threshold: float):
        """heat: as HipDetPost.launch takes it ([B, H, W], or [B, labels, H, W] whose plane 0 is the text map); tables: int32
        [B, n_angles, 2] = (c, s), every page its own (skew.coeff_table). Returns a handle for `collect`; nothing here waits."""
        assert heat.is_cuda and heat.dtype == torch.float32 and heat.is_contiguous()
        if heat.dim() == 4:
            B, Lb, H, W = heat.shape
            stride = Lb * H * W
        else:
            B, H, W = heat.shape
            stride = H * W
        tables = np.ascontiguousarray(tables, np.int32)
        assert tables.ndim == 3 and tables.shape[0] == B and tables.shape[2] == 2
        n = tables.shape[1]
        torch.cuda.set_device(self.device)
        ws, need = self._workspace(B, H, W)
        hcs = torch.empty(tables.shape, dtype=torch.int32, pin_memory=True)
        hcs.numpy()[...] = tables
        cs = hcs.to(self.device, non_blocking=True)
        scores = torch.empty((B, n), dtype=torch.int64, device=self.device)              # uint64 on the device; torch moves the bits
        n_text = torch.empty((B,), dtype=torch.int32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_skew(L.ptr(heat), stride, B, H, W, float(threshold), L.ptr(cs), n, L.ptr(scores), L.ptr(n_text), L.ptr(ws),
                                        need, stream), "surya_det_skew")
        hs = torch.empty(scores.shape, dtype=torch.int64, pin_memory=True).copy_(scores, non_blocking=True)
        hn = torch.empty(n_text.shape, dtype=torch.int32, pin_memory=True).copy_(n_text, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return (ev, hs, hn, heat, hcs, cs)              # `heat`, the tables and their staging ride along: they must outlive the kernels

    def collect(self, pending):
        """(scores uint64 [B, n_angles], n_text int32 [B]) of a launched batch."""
        ev, hs, hn = pending[:3]
        ev.synchronize()
        return hs.numpy().view(np.uint64).copy(), hn.numpy().copy()

    def __call__(self, heat: torch.Tensor, tables: np.ndarray, threshold: float):
        return self.collect(self.launch(heat, tables, threshold))


class HipDetCenterlines:
    """Centre-line profiles of the kept components on the device (surya_det_centerlines, csrc/det_centerline.h): the estimator behind
    DetectionPredictor.centerlines (detection/centerline.py states the rule and makes the curves from the integers). `launch` enqueues
    behind the surya_det_boxes call whose workspace it reads -- the HipDetPost's last launch -- and owns the output buffers; `collect` waits
    for ITS event. Of the [max_boxes] rows of every output only the first HEAD travel to the host with the launch (a page rarely has more
    lines); a page with more components fetches its rows when it is collected."""
    HEAD = 512

    def __init__(self, device="cuda:0"):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetCenterlines needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.bind_det_centerlines(L.lib())
        self.device = torch.device(device)
        self._layouts = {}

    def _comp_offset(self, B, H, W, max_boxes):
        key = (B, H, W, max_boxes)
        if key not in self._layouts:
            off = (C.c_size_t * 21)()                                # SA_DET_BOXES_LAYOUT_WORDS
            L.check(self.lib.surya_det_boxes_workspace_layout(B, H, W, max_boxes, off, 21, None, None), "surya_det_boxes_workspace_layout")
            assert int(off[20]) == 24, "CompStats is six words (csrc/det_post_core.h)"
            self._layouts[key] = int(off[12])                        # comp
        return self._layouts[key]

    def launch(self, post: HipDetPost, heat: torch.Tensor, knots: int):
        """post: the HipDetPost that has just launched on `heat` (same stream). Returns a handle for `collect`; nothing here waits."""
        B, H, W = heat.shape[0], heat.shape[-2], heat.shape[-1]
        mb = post.max_boxes
        torch.cuda.set_device(self.device)
        ws = post._ws
        need = int(self.lib.surya_det_boxes_workspace_bytes(C.c_int(B), C.c_int(H), C.c_int(W), C.c_int(mb)))
        assert ws is not None and ws.numel() >= need, "HipDetCenterlines.launch follows HipDetPost.launch of the same maps"
        dev = self.device
        cnt = torch.empty((B, mb, knots), dtype=torch.int32, device=dev)                 # uint32 / uint64 on the device; torch moves the bits
        sm = torch.empty((B, mb, knots), dtype=torch.int64, device=dev)
        lo = torch.empty((B, mb, knots), dtype=torch.int32, device=dev)
        hi = torch.empty((B, mb, knots), dtype=torch.int32, device=dev)
        axis = torch.empty((B, mb), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        L.check(self.lib.surya_det_centerlines(B, H, W, mb, int(knots), L.ptr(ws), need, L.ptr(cnt), L.ptr(sm), L.ptr(lo), L.ptr(hi), L.ptr(axis),
                                               stream), "surya_det_centerlines")
        off = self._comp_offset(B, H, W, mb)
        comp = ws[off: off + B * mb * 24].view(torch.int32).view(B, mb, 6)[:, :, :4].contiguous()      # (x0, x1, y0, y1); the next call rewrites ws
        full = (cnt, sm, lo, hi, axis, comp)
        head = min(mb, self.HEAD)
        host = tuple(torch.empty((B, head, *t.shape[2:]), dtype=t.dtype, pin_memory=True).copy_(t[:, :head], non_blocking=True) for t in full)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        return (ev, host, full, heat, post, int(knots))

    def collect(self, pending, counts, thresholds=None):
        """Per page the profile of its first counts[b] components, as detection/centerline.py `profile_page` returns it. counts: the boxes
        HipDetPost.collect returned for the same pages. A page that overflowed the post-processing's max_boxes was run again there with more
        room; its profile is taken again likewise (thresholds: the (text, low) pair of that launch)."""
        ev, host, full, heat, post, knots = pending
        ev.synchronize()
        head = host[0].shape[1]
        out = []
        over = [b for b, n in enumerate(counts) if n > post.max_boxes]
        for b, n in enumerate(counts):
            if b in over:
                out.append(None)
                continue
            src = [t[b, :n].numpy() for t in host] if n <= head else [t[b, :n].cpu().numpy() for t in full]
            cnt, sm, lo, hi, axis, box = (np.ascontiguousarray(a) for a in src)
            out.append({"cnt": cnt.view(np.uint32).copy(), "sum": sm.view(np.uint64).copy(), "lo": lo.copy(), "hi": hi.copy(), "axis": axis.copy(),
                        "box": box.copy()})
        if over:
            assert thresholds is not None, "a page overflowed max_boxes: collect needs the thresholds to run it again"
            big = HipDetPost(self.device, max_boxes=post.max_boxes * 16)
            sel = heat[over].contiguous()
            p = big.launch(sel, *thresholds)
            c = self.launch(big, sel, knots)
            redo = self.collect(c, [len(bx) for bx, _ in big.collect(p)])
            for b, r in zip(over, redo):
                out[b] = r
        return out


class DeviceResampler:
    """Pillow LANCZOS resizes (surya_resample_lanczos_u8) and integer box reductions (surya_reduce_u8) of uint8 pages on the
    device (csrc/resample.h). Coefficient tables are built once per (source length, target length, source span) by
    common/pil_resample.py and cached on the device."""

    def __init__(self, device="cuda:0"):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("DeviceResampler needs a GPU (MI355X)")
        self.lib = L.lib()
        self.device = torch.device(device)
        self._tables = {}

    def _axis(self, n_in: int, n_out: int, in0: float = 0.0, in1: float = None):
        in1 = float(n_in) if in1 is None else float(in1)
        key = (n_in, n_out, float(in0), in1)
        t = self._tables.get(key)
        if t is None:
            from ..common.pil_resample import lanczos_coeffs
            b, kk, ks = lanczos_coeffs(n_in, n_out, float(in0), in1)
            t = self._tables[key] = (torch.from_numpy(b).to(self.device), torch.from_numpy(kk).to(self.device), ks)
        return t

    def reduce(self, src: torch.Tensor, fx: int, fy: int, out: torch.Tensor = None) -> torch.Tensor:
        """src cuda uint8 [h, w, 3|4] -> Image.reduce((fx, fy)) of it as uint8 [ceil(h / fy), ceil(w / fx), out.shape[2] or 4]."""
        assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3
        h, w, sp = src.shape
        H, W = -(-h // int(fy)), -(-w // int(fx))
        if out is None:
            out = torch.empty((H, W, 4), dtype=torch.uint8, device=self.device)
        assert out.is_cuda and out.is_contiguous() and tuple(out.shape[:2]) == (H, W) and out.shape[2] in (3, 4)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_reduce_u8(L.ptr(src), C.c_int(w), C.c_int(h), C.c_int(sp), L.ptr(out), C.c_int(out.shape[2]),
                                         C.c_int(int(fx)), C.c_int(int(fy)), stream), "surya_reduce_u8")
        return out

    def resize(self, src: torch.Tensor, size, out: torch.Tensor = None, box=None) -> torch.Tensor:
        """src cuda uint8 [h, w, 3|4] -> Image.resize((W, H), LANCZOS, box) of it as uint8 [H, W, out.shape[2] or 4]. box: the
        source rectangle (x0, y0, x1, y1) of the resize that follows a reduce() (pil_resample.plan_chain), default the image."""
        assert src.is_cuda and src.dtype == torch.uint8 and src.is_contiguous() and src.dim() == 3
        h, w, sp = src.shape
        W, H = int(size[0]), int(size[1])
        x0, y0, x1, y1 = (0.0, 0.0, float(w), float(h)) if box is None else map(float, box)
        # the kernels run a pass iff the length changes; Pillow also runs one for a box that is not the whole axis, which after a
        # reduce() only comes with a length at least twice the target's
        if (W == w and (x0 != 0 or x1 != w)) or (H == h and (y0 != 0 or y1 != h)):
            raise L.SuryaAmdError(f"DeviceResampler.resize: box {box} on an axis that keeps its length ({w}x{h} -> {W}x{H})")
        if out is None:
            out = torch.empty((H, W, 4), dtype=torch.uint8, device=self.device)
        assert out.is_cuda and out.is_contiguous() and tuple(out.shape[:2]) == (H, W) and out.shape[2] in (3, 4)
        bx = kx = by = ky = None
        ksx = ksy = 0
        if W != w:
            bx, kx, ksx = self._axis(w, W, x0, x1)
        if H != h:
            by, ky, ksy = self._axis(h, H, y0, y1)
        tmp = torch.empty((h, W, 4), dtype=torch.uint8, device=self.device) if (W != w and H != h) else None
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_resample_lanczos_u8(L.ptr(src), C.c_int(w), C.c_int(h), C.c_int(sp), L.ptr(out), C.c_int(W), C.c_int(H),
                                                   C.c_int(out.shape[2]), L.ptr(bx), L.ptr(kx), C.c_int(ksx), L.ptr(by), L.ptr(ky),
                                                   C.c_int(ksy), L.ptr(tmp), stream), "surya_resample_lanczos_u8")
        return out


# must match sa::tile::CutDesc / StitchDesc (csrc/det_tile.h, include/surya_amd.h): DEVICE tables, one entry per tile
CUT_DESC = np.dtype([("src", "<u8"), ("w", "<i4"), ("h", "<i4"), ("pix", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("tile", "<i4")])
STITCH_DESC = np.dtype([("dst", "<u8"), ("pitch", "<i8"), ("plane_stride", "<i8"), ("tile", "<i4"), ("tx0", "<i4"), ("ty0", "<i4"),
                        ("tw", "<i4"), ("th", "<i4"), ("dx0", "<i4"), ("dy0", "<i4"), ("planes", "<i4"), ("pad_cols", "<i4"),
                        ("reserved", "<i4")])
assert CUT_DESC.itemsize == 32 and STITCH_DESC.itemsize == 64


class HipDetTiler:
    """The two copies of tiled detection (surya_det_cut_tiles_u8, surya_det_stitch_tiles; csrc/det_tile.h): windows of uint8 pages ->
    the tile batch `forward_u8` reads, and the rectangle every tile owns of its heat planes -> the page map. Descriptor tables are
    device memory (a uint8 tensor holding CUT_DESC / STITCH_DESC records); the predictor uploads them with the pages."""

    def __init__(self, device="cuda:0"):
        if not torch.cuda.is_available():
            raise L.SuryaAmdError("HipDetTiler needs a GPU (MI355X); there is no CPU fallback")
        self.lib = L.bind_det_tile(L.lib())
        self.device = torch.device(device)

    def table(self, descs: np.ndarray) -> torch.Tensor:
        """A host descriptor array as a device table (op-level callers; the predictor packs its tables into the batch's staging buffer)."""
        assert descs.dtype in (CUT_DESC, STITCH_DESC)
        return torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8).copy()).to(self.device)

    def cut(self, table: torch.Tensor, n: int, dst: torch.Tensor):
        """table: device uint8, n CUT_DESC records; dst: cuda uint8 [tiles, P, P, 3 | 4], written in place."""
        assert table.is_cuda and table.dtype == torch.uint8 and table.numel() >= n * CUT_DESC.itemsize and table.data_ptr() % 8 == 0
        assert dst.is_cuda and dst.dtype == torch.uint8 and dst.is_contiguous() and dst.dim() == 4 and dst.shape[1] == dst.shape[2]
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_cut_tiles_u8(L.ptr(table), n, L.ptr(dst), dst.shape[0], dst.shape[1], dst.shape[3], stream),
                "surya_det_cut_tiles_u8")

    def stitch(self, heat: torch.Tensor, table: torch.Tensor, n: int):
        """heat: cuda fp32 [tiles, labels, P, P]; table: device uint8, n STITCH_DESC records naming the page maps."""
        assert table.is_cuda and table.dtype == torch.uint8 and table.numel() >= n * STITCH_DESC.itemsize and table.data_ptr() % 8 == 0
        assert heat.is_cuda and heat.dtype == torch.float32 and heat.is_contiguous() and heat.dim() == 4 and heat.shape[2] == heat.shape[3]
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        L.check(self.lib.surya_det_stitch_tiles(L.ptr(heat), heat.shape[0], heat.shape[1], heat.shape[2], L.ptr(table), n, stream),
                "surya_det_stitch_tiles")
