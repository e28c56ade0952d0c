"""LRPEngine — thin Python owner of one `lrp_handle` (one per GPU / stream).

PyTorch is plumbing only: it owns the device tensors that cross the C ABI
(images, relevance maps) and the current stream.  All arithmetic of the hot
path runs in liblrp_hip.so.
"""
import ctypes as C

import numpy as np
import torch

from . import _capi
from .synthetic import VGG16_CFG


def _i32(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


class LRPEngine(object):
    """Geometry + weights + caches for one captioning model on one GPU."""

    def __init__(self, decoder="adaptive", cnn_cfg=VGG16_CFG, img_hw=(224, 224), L=196, D=512, H=512, E=512,
                 V=10000, max_images=32, max_tokens=320, max_caption_len=21, sos_id=2, eos_id=1, device=None,
                 resnet=None):
        """resnet: None (VGG-style `cnn_cfg`) or dict(stem=64, stacks=((64,3),(128,4),(256,23),(512,3))) for the
        ResNet-v1 bottleneck encoder of BASELINE config 4 (then cnn_cfg is ignored)."""
        if decoder not in ("adaptive", "gridtd"):
            raise NotImplementedError("decoder must be 'adaptive' or 'gridtd'")
        self._lib = _capi.load()                      # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise RuntimeError("LRPEngine needs a ROCm GPU (no CPU fallback for the LRP hot path)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        cfg = _capi.LrpConfig()
        cfg.abi_version = _capi.LRP_ABI_VERSION
        cfg.device = self.device.index
        cfg.decoder = _capi.LRP_DEC_ADAPTIVE if decoder == "adaptive" else _capi.LRP_DEC_GRIDTD
        cfg.img_h, cfg.img_w = img_hw
        if resnet is None:
            cfg.encoder = _capi.LRP_ENC_VGG
            cfg.n_conv = len(cnn_cfg)
            for i, (name, cin, cout, pool) in enumerate(cnn_cfg):
                cfg.conv_cin[i], cfg.conv_cout[i], cfg.conv_pool_after[i] = cin, cout, int(bool(pool))
                cfg.conv_name[i].value = name.encode()
        else:
            cfg.encoder = _capi.LRP_ENC_RESNET
            cfg.resnet_stem = int(resnet.get("stem", 64))
            stacks = list(resnet["stacks"])
            cfg.resnet_n_stacks = len(stacks)
            for i, (f, nb) in enumerate(stacks):
                cfg.resnet_filters[i], cfg.resnet_blocks[i] = int(f), int(nb)
        cfg.L, cfg.D, cfg.H, cfg.E, cfg.V = L, D, H, E, V
        cfg.max_images, cfg.max_tokens, cfg.max_caption_len = max_images, max_tokens, max_caption_len
        cfg.sos_id, cfg.eos_id = sos_id, eos_id
        self.cfg = cfg
        self.decoder = decoder
        self.cnn_cfg = list(cnn_cfg)
        self.img_hw = tuple(img_hw)
        self.L, self.D, self.H, self.E, self.V = L, D, H, E, V
        self.max_images, self.max_tokens, self.Tm = max_images, max_tokens, max_caption_len
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _capi.check(self._lib.lrp_create(C.byref(cfg), C.byref(self._h)))
        self.captions = None
        self.n_images = 0
        self.precision = "bf16x3"                       # library default for the reverse walk (set_precision)
        self.cnn_rule = (1, 0)                          # ... and for its conv rule (set_cnn_rule)
        self.cnn_rules = None                           # ... or the table in its place (set_cnn_rules; ResNet: the pair (stem, units))

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.lrp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def workspace_bytes(self):
        return int(self._lib.lrp_workspace_bytes(self._h))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype=torch.float32):
        if isinstance(x, torch.Tensor):
            return x.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(self.device)

    # ------------------------------------------------------------------ weights
    def set_weights(self, weights):
        """weights: dict name -> float32 array in the Keras layout (conv HWIO, dense (in,out))."""
        for name, arr in weights.items():
            if isinstance(arr, torch.Tensor):
                arr = arr.detach().cpu().numpy()
            a = np.ascontiguousarray(arr, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            _capi.check(self._lib.lrp_set_weight(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), a.ndim, shape))

    def set_weights_from_device(self, weights):
        """Same, from CUDA tensors (e.g. after an RCCL broadcast of the frozen bundle)."""
        for name, t in weights.items():
            t = t.to(device=self.device, dtype=torch.float32).contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            _capi.check(self._lib.lrp_set_weight_dev(self._h, name.encode(), C.c_void_p(t.data_ptr()), t.dim(), shape,
                                                     self._stream()))

    # ------------------------------------------------------------------ encoder
    def encode_images(self, images):
        """images (B,H,W,3) float32 BGR mean-subtracted -> caches; returns nothing."""
        x = self._dev(images)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_hw[0], self.img_hw[1], 3):
            raise ValueError("images must be (B,%d,%d,3)" % self.img_hw)
        _capi.check(self._lib.lrp_encode_images(self._h, C.c_void_p(x.data_ptr()), x.shape[0], self._stream()))
        self.n_images = int(x.shape[0])
        self.captions = None

    def set_features(self, feat):
        f = self._dev(feat).reshape(-1, self.L, self.D)
        _capi.check(self._lib.lrp_set_features(self._h, C.c_void_p(f.data_ptr()), f.shape[0], self._stream()))
        self.n_images = int(f.shape[0])
        self.captions = None

    def get_features(self):
        out = torch.empty((self.n_images, self.L, self.D), dtype=torch.float32, device=self.device)
        _capi.check(self._lib.lrp_get_features(self._h, C.c_void_p(out.data_ptr()), self.n_images, self._stream()))
        return out

    # ------------------------------------------------------------------ decoder
    def decoder_forward(self, captions):
        """captions: list (per image) of tokenizer-id lists ending in EOS."""
        B = len(captions)
        caps = np.full((B, self.Tm), int(self.cfg.eos_id), dtype=np.int32)
        lens = np.zeros((B,), dtype=np.int32)
        for b, c in enumerate(captions):
            if len(c) > self.Tm:
                raise ValueError("caption %d longer than max_caption_len=%d" % (b, self.Tm))
            caps[b, :len(c)] = c
            lens[b] = len(c)
        caps, pc = _i32(caps)
        lens, pl = _i32(lens)
        _capi.check(self._lib.lrp_decoder_forward(self._h, pc, pl, B, self._stream()))
        self.captions = [list(map(int, c)) for c in captions]

    _STATE_SHAPES = {
        "ht": ("S", "H", torch.float32), "ct": ("S", "H", torch.float32), "gt": ("S", "H", torch.float32),
        "it_act": ("S", "H", torch.float32), "ft_act": ("S", "H", torch.float32), "st": ("S", "H", torch.float32),
        "ot_act": ("S", "H", torch.float32),
        "attention": ("S", "L", torch.float32), "beta": ("S", 1, torch.float32),
        "context": ("S", "H", torch.float64), "c_hat": ("S", "H", torch.float64),
        "xt": ("T", "2E", torch.float32), "caption_preds": ("T", "V", torch.float64),
        "image_features_before_act": ("L", "H", torch.float32), "average_img_feature": (1, "D", torch.float32),
        "global_img_feature_before_act": (1, "E", torch.float32), "total_static_img_feature": ("L", "H", torch.float32),
    }

    _STATE_SHAPES_GRIDTD = dict(
        [(n, ("S", "H", torch.float64)) for n in ("h1t", "c1t", "g1t", "i1t_act", "f1t_act", "h2t", "c2t", "g2t", "i2t_act",
                                                  "f2t_act", "context", "st", "context_hat", "o1t_act", "o2t_act")] +
        [("attention", ("S", "L", torch.float64)), ("beta", ("S", 1, torch.float64)),
         ("x1t", ("T", "H+2E", torch.float64)), ("x2t", ("T", "2H", torch.float64)),
         ("caption_preds", ("T", "V", torch.float64)),
         ("image_features_before_act", ("L", "H", torch.float32)), ("average_img_feature", (1, "D", torch.float32)),
         ("global_img_feature_before_act", (1, "E", torch.float32)), ("image_features_proj", ("L", "H", torch.float32))])

    def read_state(self, name):
        """Cached decoder array for the images of the last forward: (B, rows, dim)."""
        dims = {"S": self.Tm + 1, "T": self.Tm, "H": self.H, "L": self.L, "V": self.V, "D": self.D, "E": self.E,
                "2E": 2 * self.E, "2H": 2 * self.H, "H+2E": self.H + 2 * self.E, 1: 1}
        r, c, dt = (self._STATE_SHAPES_GRIDTD if self.decoder == "gridtd" else self._STATE_SHAPES)[name]
        out = torch.empty((self.n_images, dims[r], dims[c]), dtype=dt, device=self.device)
        _capi.check(self._lib.lrp_read_state(self._h, name.encode(), C.c_void_p(out.data_ptr()),
                                             out.numel() * out.element_size(), self._stream()))
        return out

    def decoder_explain(self, img_idx, t, variant="sequence", want_attention=True, want_r_words=True):
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        tt, pt = _i32(t)
        R = torch.empty((n, self.L, self.D), dtype=torch.float32, device=self.device)
        att = torch.empty((n, self.L), dtype=torch.float32, device=self.device) if want_attention else None
        rw = torch.empty((n, self.Tm), dtype=torch.float64, device=self.device) if want_r_words else None
        v = _capi.LRP_EXPLAIN_SEQUENCE if variant == "sequence" else _capi.LRP_EXPLAIN_SINGLE_STEP
        _capi.check(self._lib.lrp_decoder_explain(
            self._h, n, pi, pt, v, C.c_void_p(R.data_ptr()),
            C.c_void_p(att.data_ptr()) if att is not None else None,
            C.c_void_p(rw.data_ptr()) if rw is not None else None, self._stream()))
        return R, att, rw

    # ------------------------------------------------------------------ CNN LRP
    def cnn_explain(self, img_idx, R_feat, out=None):
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        R = self._dev(R_feat).reshape(n, self.L, self.D)
        if out is None:
            out = torch.empty((n, self.img_hw[0], self.img_hw[1], 3), dtype=torch.float32, device=self.device)
        _capi.check(self._lib.lrp_cnn_explain(self._h, n, pi, C.c_void_p(R.data_ptr()), C.c_void_p(out.data_ptr()),
                                              self._stream()))
        return out

    # ------------------------------------------------------------------ layer trace
    def set_layer_trace(self, on):
        """The trace switch of a VGG-style engine (lrp_set_layer_trace): while on, encode_images keeps every conv's input and
        cnn_explain_traced runs.  A change drops the encode caches: call encode_images again.  NotImplementedError on a
        ResNet engine."""
        on = bool(on)
        _capi.check(self._lib.lrp_set_layer_trace(self._h, int(on)))
        if on != getattr(self, "layer_trace", False):
            self.n_images = 0                            # the library dropped the caches
            self.captions = None
        self.layer_trace = on

    def _trace_info(self, n, mask):
        """[(nid, (H, W, C), offset)] in sorted-id order and the keep buffer's size in floats, for n rows and `mask`"""
        cnt = int(self._lib.lrp_trace_tensor_count(self._h))
        if cnt < 0:
            _capi.check(cnt)
        vals = [C.c_int32() for _ in range(4)]
        off, tot = C.c_int64(), C.c_int64()
        out = []
        for i in range(cnt):
            _capi.check(self._lib.lrp_trace_tensor_info(self._h, i, n, mask, *[C.byref(v) for v in vals], C.byref(off), C.byref(tot)))
            out.append((vals[0].value, (vals[1].value, vals[2].value, vals[3].value), off.value))
        return out, tot.value

    def trace_tensors(self):
        """The traced tensors in sorted-id order, as the reference names its reversed tensors: [((nid, 0), (H, W, C))] —
        (-1, 0) the head, (nid, 0) the relevance at the input of node nid (convs and 2x2 pools in execution order), (0, 0) the
        image-level result."""
        return [((nid, 0), shape) for nid, shape, _ in self._trace_info(1, 0)[0]]

    def cnn_explain_traced(self, img_idx, R_feat, keep=(), out=None):
        """cnn_explain with the relevance at every layer's input (lrp_cnn_explain_traced; needs set_layer_trace(True) and an
        encode since).  keep: ids (nid, 0) or node ids of the tensors to return, True for all (False / None / (): none).  Returns (R_img, stats, kept):
        stats (n_tensors, n, 4) float64 — minimum, maximum, sum, non-finite count per tensor (trace_tensors() order) and row;
        kept: dict id -> (n, H, W, C) float32 tensor (views of one buffer)."""
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        R = self._dev(R_feat).reshape(n, self.L, self.D)
        ids = [nid for nid, _, _ in self._trace_info(1, 0)[0]]
        if keep is True:
            want = list(ids)
        elif keep is False or keep is None:
            want = []
        else:
            want = [int(k[0]) if isinstance(k, (tuple, list)) else int(k) for k in keep]
            for k in want:
                if k not in ids:
                    raise ValueError("no traced tensor (%d, 0): ids are (-1, 0) .. (%d, 0)" % (k, ids[-1]))
        mask = sum(1 << ids.index(k) for k in set(want))
        info, total = self._trace_info(n, mask)
        if out is None:
            out = torch.empty((n, self.img_hw[0], self.img_hw[1], 3), dtype=torch.float32, device=self.device)
        stats = torch.empty((len(ids), n, 4), dtype=torch.float64, device=self.device)
        buf = torch.empty((max(total, 1),), dtype=torch.float32, device=self.device) if mask else None
        _capi.check(self._lib.lrp_cnn_explain_traced(self._h, n, pi, C.c_void_p(R.data_ptr()), C.c_void_p(out.data_ptr()),
                                                     C.c_void_p(stats.data_ptr()), mask,
                                                     C.c_void_p(buf.data_ptr()) if buf is not None else None, total, self._stream()))
        kept = {}
        for nid, (H, W, Cc), off in info:
            if off >= 0:
                kept[(nid, 0)] = buf[off:off + n * H * W * Cc].view(n, H, W, Cc)
        return out, stats, kept

    def tensor_stats(self, x):
        """Minimum, maximum, float64 sum and non-finite count of every row of x (rows, ...) float32 on the device
        (lrp_op_tensor_stats): (rows, 4) float64.  min / max are NaN where the row holds a NaN; -0.0 orders below +0.0."""
        x = self._dev(x)
        if x.dim() < 1 or x.numel() == 0:
            raise ValueError("x must be a non-empty (rows, ...) array")
        rows = int(x.shape[0])
        stats = torch.empty((rows, 4), dtype=torch.float64, device=self.device)
        _capi.check(self._lib.lrp_op_tensor_stats(C.c_void_p(x.data_ptr()), rows, x.numel() // rows, C.c_void_p(stats.data_ptr()),
                                                  self._stream()))
        return stats

    # ------------------------------------------------------------------ fine-tune step
    def train_begin(self, lr=2e-4, clipvalue=0.01, beta1=0.9, beta2=0.999, eps=1e-7):
        """Adam(lr, clipvalue) as `ImgCaptioningAdaptiveAttentionLRPInferenceModel.build` compiles it (M:1370);
        returns the layout of the flat parameter / gradient buffers: {name: (offset, size)}."""
        _capi.check(self._lib.lrp_train_begin(self._h, C.c_float(lr), C.c_float(clipvalue), C.c_float(beta1), C.c_float(beta2),
                                              C.c_float(eps)))
        self.train_flat_size = int(self._lib.lrp_train_flat_size(self._h))
        self.train_layout = {}
        for i in range(int(self._lib.lrp_train_num_params(self._h))):
            nm, off, n = C.c_char_p(), C.c_int64(), C.c_int64()
            _capi.check(self._lib.lrp_train_param_info(self._h, i, C.byref(nm), C.byref(off), C.byref(n)))
            self.train_layout[nm.value.decode()] = (int(off.value), int(n.value))
        self.n_images = 0
        return self.train_layout

    def train_set_precision(self, mode):
        """'fp32' (default: fp32-grade gradients) or 'bf16' (BASELINE config 5: the encoder's weight gradients with bf16
        operands, fp32 accumulation and fp32 master weights) — lrp_train_set_precision."""
        m = {"fp32": _capi.LRP_TRAIN_FP32, "bf16": _capi.LRP_TRAIN_BF16}.get(mode)
        if m is None:
            raise ValueError("training precision must be 'fp32' or 'bf16'")
        _capi.check(self._lib.lrp_train_set_precision(self._h, m))
        self.train_precision = mode

    def _train_inputs(self, cap_in, masks, pending=None):
        """Device copies + checks of what the decoder's training forward reads: cap_in (B, T) and the dropout masks.
        pending: what a not yet consumed train_forward converted — the same source OBJECT maps to the same device tensor
        (lrp_train_step insists on the pointers lrp_train_forward read)."""
        masks = masks or {}
        cache = pending or {}
        made = {}
        hit = cache.get("cap_in")
        ci = hit[1] if hit is not None and hit[0] is cap_in else self._dev(cap_in, torch.int32)
        if hit is not None and hit[0] is cap_in:
            ci.record_stream(torch.cuda.current_stream(self.device))
        made["cap_in"] = (cap_in, ci)
        if ci.dim() != 2:
            raise ValueError("cap_in must be (B, T)")
        B, T = ci.shape
        # the kernels index the embedding / the logits with these: validate on the host side of the boundary
        if int(ci.min()) < 0 or int(ci.max()) >= self.V:
            raise ValueError("cap_in holds embedding rows outside [0, V)")
        if B > self.n_images:
            raise RuntimeError("encode_images must run on the batch before the fine-tune step")
        for k in masks:
            if k not in ("image_features", "global", "output", "lstm_in", "lstm_rec", "logits"):
                raise ValueError("unknown dropout mask '%s'" % k)
        self._train_made = made

        def m(key, shape):
            src = masks.get(key)
            if src is None:
                return None
            hit = cache.get(key)
            if hit is not None and hit[0] is src:
                v = hit[1]
                v.record_stream(torch.cuda.current_stream(self.device))      # (made under the early forward's stream)
            else:
                v = self._dev(src)
            made[key] = (src, v)
            if tuple(v.shape) != shape:
                raise ValueError("mask '%s' must be %s" % (key, shape))
            return v
        win = 2 * self.H if self.decoder == "gridtd" else 2 * self.E         # language LSTM input [c_hat | h1] / [emb | glob]
        return ci, (m("image_features", (B, self.L, self.H)), m("global", (B, self.E)), m("output", (B, T, self.H)),
                    m("lstm_in", (T, 4, B, win)), m("lstm_rec", (T, 4, B, self.H)), m("logits", (B, T, self.V)))

    def train_forward(self, cap_in, masks=None):
        """The training-mode decoder forward of `train_step`, ahead of time on the CURRENT stream (it needs neither
        lrp_weight nor the labels): issue it on a side stream under the explanation that produces lrp_weight; the next
        `train_step` with the same (B, T) waits for it and starts at the loss.  Pass the same cap_in / masks to both."""
        ci, (mi, mg, mo, ml, mr, _) = self._train_inputs(cap_in, masks)
        B, T = ci.shape
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _capi.check(self._lib.lrp_train_forward(self._h, B, T, p(ci), p(mi), p(mg), p(mo), p(ml), p(mr), self._stream()))
        self._train_fwd_keep = self._train_made                             # alive (and reused) until the step has consumed them

    def train_step(self, cap_in, y_idx, lrp_weight, masks=None, grads=None):
        """Gradients of the two-headed loss for the images last encoded.  cap_in / y_idx (B, T) ints (y -1 = no label),
        lrp_weight (B, T, V).  masks: dict with optional 'image_features' (B, L, H), 'global' (B, E), 'output' (B, T, H),
        'lstm_in' (T, 4, B, 2E), 'lstm_rec' (T, 4, B, H) (the LSTM cell's per-gate, per-step dropout).
        Returns (grads flat float32 device tensor, losses (5,) device tensor = total, loss head 1, loss head 2,
        accuracy head 1, accuracy head 2: the list `train_on_batch` returns)."""
        try:
            ci, (mi, mg, mo, ml, mr, mz) = self._train_inputs(cap_in, masks, getattr(self, "_train_fwd_keep", None))
            yi = self._dev(y_idx, torch.int32)
            B, T = ci.shape
            lw = self._dev(lrp_weight).reshape(B, T, self.V)
            if tuple(yi.shape) != (B, T):
                raise ValueError("y_idx must have the shape of cap_in")
            if int(yi.min()) < -1 or int(yi.max()) >= self.V:
                raise ValueError("y_idx holds class indices outside [-1, V)")
            if grads is None:
                grads = torch.empty(self.train_flat_size, dtype=torch.float32, device=self.device)
            losses = torch.empty(5, dtype=torch.float32, device=self.device)
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
            _capi.check(self._lib.lrp_train_step(self._h, B, T, p(ci), p(yi), p(lw), p(mi), p(mg), p(mo), p(ml), p(mr), p(mz),
                                                 p(grads), p(losses), self._stream()))
        except Exception:
            # A refused / failed step must not leave the library holding pointers of an early forward whose device tensors
            # are about to lose their keep-alive: torch would hand the same addresses to a retry's fresh masks and the
            # pointer comparison in lrp_train_step would pass for buffers the forward never read.  Drop it first (the
            # stream waits for the early forward), THEN release the tensors.
            self._lib.lrp_train_drop_forward(self._h, self._stream())
            self._train_fwd_keep = None
            raise
        self._train_fwd_keep = None                                         # consumed: the step's work is stream-ordered behind it
        return grads, losses

    def train_apply(self, grads):
        """Adam update of the master weights from the (all-reduced) flat gradient; cached images are dropped."""
        _capi.check(self._lib.lrp_train_apply(self._h, C.c_void_p(grads.data_ptr()), self._stream()))
        self.n_images = 0
        self.captions = None

    def train_weights_device(self):
        """Master weights as {name: flat float32 device view} of one fresh copy of the flat buffer."""
        flat = torch.empty(self.train_flat_size, dtype=torch.float32, device=self.device)
        _capi.check(self._lib.lrp_train_get_master(self._h, C.c_void_p(flat.data_ptr()), self._stream()))
        return {k: flat[o:o + n] for k, (o, n) in self.train_layout.items()}

    def train_weights(self):
        """Master weights as {name: float32 ndarray} (checkpointing / tests)."""
        return {k: v.cpu().numpy().copy() for k, v in self.train_weights_device().items()}

    # ------------------------------------------------------------------ caption generation
    def gen_begin(self, n_rows):
        """Start an incremental decode over the first n_rows cached feature slots (one hypothesis per row)."""
        _capi.check(self._lib.lrp_decoder_gen_begin(self._h, int(n_rows), self._stream()))
        self._gen_rows = int(n_rows)

    def gen_step(self, step, parent=None, word=None):
        """One decoder step for every row; row r continues row parent[r] with tokenizer id word[r] appended
        (step 0: SOS).  Returns the (n_rows, V) float64 logits of position `step` on the device."""
        n = self._gen_rows
        out = torch.empty((n, self.V), dtype=torch.float64, device=self.device)
        if step > 0:
            pp, ppi = _i32(parent)
            ww, wwi = _i32(word)
        else:
            ppi = wwi = None
        _capi.check(self._lib.lrp_decoder_gen_step(self._h, n, ppi, wwi, int(step), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def log_softmax_topk(self, logits, k):
        """`_log_softmax` + `np.argpartition(preds, -k)[:, -k:]` (explainers.py:45-48, :76-78) on the device for the
        (rows, V) float64 logits of `gen_step`: (ids (rows, k) int32 model columns, logp (rows, k) float64), both by
        descending probability.  Only these k pairs per row have to cross PCIe."""
        return log_softmax_topk(logits, k)

    def _beam_search_packed(self, n_images, k, steps, eos):
        """lrp_decoder_beam_search into ONE device allocation: (buffer, (captions, lengths, logp, n_complete) views)."""
        n, k = int(n_images), int(k)
        if n < 1 or k < 1:
            raise ValueError("n_images and k must be positive")
        buf, views = _beam_result_views(n, k, self.Tm, self.device)
        p = lambda t: C.c_void_p(t.data_ptr())
        _capi.check(self._lib.lrp_decoder_beam_search(self._h, n, k, int(steps), int(eos), p(views[0]), p(views[1]), p(views[2]),
                                                      p(views[3]), self._stream()))
        return buf, views

    def beam_search(self, n_images, k, steps, eos):
        """The whole caption search of explainers.py:51-120 on the stream, after `gen_begin(n_images * k)` on features laid
        out one slot per (image, beam): `steps` decoder steps with the ranking and the beam bookkeeping on the device, no
        host round trip in between.  Returns device tensors: captions (n_images, k, max_caption_len + 1) int32 tokenizer
        ids with a trailing EOS, zero-padded (complete captions by descending order, then live ones: what `beam.search`
        returns; [:, 0] is the reference's answer), lengths (n_images, k) int32, logp (n_images, k) float64,
        n_complete (n_images,) int32."""
        return self._beam_search_packed(n_images, k, steps, eos)[1]

    def beam_search_lists(self, n_images, k, steps, eos):
        """`beam_search`, brought to the host in one copy, in the form `beam.search` returns: per image a list of captions."""
        buf, _ = self._beam_search_packed(n_images, k, steps, eos)
        caps, lens, _, _ = _beam_result_views(int(n_images), int(k), self.Tm, None, buf.cpu())[1]
        return beam_lists(caps, lens)

    # ------------------------------------------------------------------ gradient baselines
    WALKS = {"lrp": 0, "gradient": 1, "input_x_gradient": 2, "guided_backprop": 3, "deconvnet": 4, "deeplift": 5,
             "patternnet": 6, "pattern_attribution": 7}

    def decoder_gradient(self, img_idx, t, want_r_words=True):
        """_lstm_decoder_backward (explainers.py:780-832 / :1452-1532) for n (image, t) units: (n, L, D) float32
        and the per-word sums r_words (n, Tm) float64 (columns >= t are zero)."""
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        tt, pt = _i32(t)
        d = torch.empty((n, self.L, self.D), dtype=torch.float32, device=self.device)
        rw = torch.zeros((n, self.Tm), dtype=torch.float64, device=self.device) if want_r_words else None
        _capi.check(self._lib.lrp_decoder_gradient(self._h, n, pi, pt, C.c_void_p(d.data_ptr()),
                                                   C.c_void_p(rw.data_ptr()) if rw is not None else None, self._stream()))
        return d, rw

    def cnn_walk(self, img_idx, head, walk="gradient", out=None):
        """Gradient / InputTimesGradient / GuidedBackprop `.analyze([X, head])` (gradient_based.py:101-265) on the
        cached forward of `lrp_encode_images`; walk='lrp' is cnn_explain; walk='deconvnet' (gradient_based.py:180-225) reads
        no ReLU decision of the forward and runs in every precision mode on both encoders; 'patternnet' / 'pattern_attribution'
        (pattern_based.py:68-281) run on the patterns of pattern_fit / set_patterns, VGG-style engines in 'fp32' mode only."""
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        Hd = self._dev(head).reshape(n, self.L, self.D)
        if out is None:
            out = torch.empty((n, self.img_hw[0], self.img_hw[1], 3), dtype=torch.float32, device=self.device)
        _capi.check(self._lib.lrp_cnn_walk(self._h, n, pi, C.c_void_p(Hd.data_ptr()), C.c_void_p(out.data_ptr()),
                                           self.WALKS[walk], self._stream()))
        return out

    AUGMENT_KINDS = ("gaussian", "path")

    def cnn_walk_augmented(self, images, head, walk, kind, n, noise_scale=1.0, seed=0, reference=0, path="reference",
                           postprocess=None, max_batch=None):
        """GaussianSmoother / PathIntegrator (wrapper.py:214-345) around an encoder walk, on the device: for the (B, H, W, 3)
        images and their (B, L, D) heads, the B * n samples (kind 'gaussian': x + noise_scale * N(seed); 'path': the path of
        op_augment_path) are explained in chunks of at most min(max_images, max_tokens, max_batch) samples — augment ->
        encode_images(chunk) -> cnn_walk(chunk rows, the head of each row's image, walk) -> accumulate — and reduced to the
        per-image mean of postprocess(map) (None / 'abs' / 'square'), for 'path' times (x - reference).  Chunks may cross
        image boundaries; the result does not depend on the chunk size.  walk: any name of WALKS; under 'input_x_gradient'
        the product is with the SAMPLE, as the reference's subanalyzer sees the augmented input.  Only the returned (B, H, W, 3)
        float32 tensor is ever meant to leave the device.
        The call overwrites the handle's encode caches with samples: afterwards they belong to no image (n_images = 0,
        captions = None) and encode_images has to run again before anything else is explained."""
        if walk not in self.WALKS:
            raise ValueError("unknown walk %r: one of %s" % (walk, sorted(self.WALKS)))
        if walk == "deeplift":
            raise TypeError("the DeepLIFT walk is not built under an augmenting wrapper")
        if kind not in self.AUGMENT_KINDS:
            raise ValueError("kind must be 'gaussian' or 'path'")
        if postprocess not in _POST:
            raise ValueError("Parameter 'postprocess' must be either None, 'abs', or 'square'.")
        if path not in ("reference", "standard"):
            raise ValueError("path must be 'reference' or 'standard'")
        n = int(n)
        if n < 1:
            raise ValueError("the number of samples per image must be at least 1")
        x = self._dev(images)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_hw[0], self.img_hw[1], 3):
            raise ValueError("images must be (B,%d,%d,3)" % self.img_hw)
        B = int(x.shape[0])
        Hd = self._dev(head).reshape(-1, self.L, self.D)
        if Hd.shape[0] != B:
            raise ValueError("X and head must have the same batch size")
        chunk = min(self.max_images, self.max_tokens, int(max_batch) if max_batch else self.max_images)
        if chunk < 1:
            raise ValueError("max_batch must be at least 1")
        acc = torch.zeros(x.shape, dtype=torch.float64, device=self.device)
        samples = torch.empty((chunk,) + tuple(x.shape[1:]), dtype=torch.float32, device=self.device)
        maps = torch.empty_like(samples)
        try:
            for r0 in range(0, B * n, chunk):
                cnt = min(chunk, B * n - r0)
                if kind == "gaussian":
                    op_augment_gaussian(x, n, noise_scale, seed, r0, cnt, out=samples[:cnt])
                else:
                    op_augment_path(x, n, reference, path, r0, cnt, out=samples[:cnt])
                self.encode_images(samples[:cnt])
                rows = torch.arange(r0, r0 + cnt, device=self.device) // n
                self.cnn_walk(list(range(cnt)), Hd.index_select(0, rows), walk, out=maps[:cnt])
                op_reduce_accumulate(maps[:cnt], acc, n, r0, postprocess)
        finally:
            self.n_images = 0
            self.captions = None
        return op_reduce_finish(acc, n, x if kind == "path" else None, reference)

    def guided_gradcam(self, img_idx, t, want_cam=False):
        """Guided Grad-CAM (explainers.py:930-949 / :1634-1653) for n <= max_tokens (image, t) units in one chain on the
        cached forward: decoder_gradient -> cnn_walk('guided_backprop') -> op_gradcam on get_features().  Returns the
        (n, H, W, 3) float64 tensor `guided backprop * cam` (and the (n, H, W) float64 cams); nothing leaves the device."""
        g = int(round(np.sqrt(self.L)))
        up = self.img_hw[0] // max(g, 1)
        if g * g != self.L or g * up != self.img_hw[0] or self.img_hw[0] != self.img_hw[1]:
            raise ValueError("guided_gradcam needs a square image whose side is a multiple of sqrt(L)")
        if len(img_idx) != len(t) or not 1 <= len(img_idx) <= self.max_tokens:
            raise ValueError("need between 1 and max_tokens=%d (image, t) units" % self.max_tokens)
        d, _ = self.decoder_gradient(img_idx, t, want_r_words=False)
        gb = self.cnn_walk(img_idx, d, "guided_backprop")
        out, cam = op_gradcam(self.get_features(), img_idx, d, g, up, gb=gb)
        return (out, cam) if want_cam else out

    def explain_tokens(self, img_idx, t, variant="sequence", out=None, want_R_feat=False, want_attention=False,
                       want_r_words=False):
        """Fused decoder-LRP -> CNN-LRP for n (image, t) pairs: (n,H,W,3) heat-map relevances."""
        n = len(img_idx)
        ii, pi = _i32(img_idx)
        tt, pt = _i32(t)
        if out is None:
            out = torch.empty((n, self.img_hw[0], self.img_hw[1], 3), dtype=torch.float32, device=self.device)
        R = torch.empty((n, self.L, self.D), dtype=torch.float32, device=self.device) if want_R_feat else None
        att = torch.empty((n, self.L), dtype=torch.float32, device=self.device) if want_attention else None
        rw = torch.empty((n, self.Tm), dtype=torch.float64, device=self.device) if want_r_words else None
        v = _capi.LRP_EXPLAIN_SEQUENCE if variant == "sequence" else _capi.LRP_EXPLAIN_SINGLE_STEP
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
        _capi.check(self._lib.lrp_explain_tokens(self._h, n, pi, pt, v, p(out), p(R), p(att), p(rw), self._stream()))
        return out, R, att, rw

    def set_precision(self, mode):
        """'bf16x3' (default: split-bf16 walk, hi*hi' + hi*lo' + lo*hi' in every layer, 16 mantissa bits on both operands —
        parity independent of the weight statistics), 'fp32' (exact fp32 MFMA, the reference's arithmetic), 'f16x2'
        (opt-in fast mode: fp16-pair relevance, ONE fp16 per weight below the top block — two MFMAs per product; its error
        depends on how concentrated the weights are, see include/lrp_hip.h) or 'bf16x3_fast' (split forward activations
        too).  A mode change drops the encode caches: call encode_images again."""
        m = {"fp32": _capi.LRP_PREC_FP32, "bf16x3": _capi.LRP_PREC_BF16X3, "bf16x3_fast": _capi.LRP_PREC_BF16X3_FAST,
             "f16x2": _capi.LRP_PREC_F16X2}.get(mode)
        if m is None:
            raise ValueError("precision must be 'fp32', 'bf16x3', 'bf16x3_fast' or 'f16x2'")
        _capi.check(self._lib.lrp_set_precision(self._h, m))
        if mode != self.precision:
            self.n_images = 0                            # the library dropped the caches of the other arithmetic
            self.captions = None
        self.precision = mode

    def set_cnn_rule(self, alpha=None, beta=None):
        """The conv rule of the encoder's LRP walk (lrp_set_cnn_rule), VGG-style or ResNet: AlphaBetaRule with alpha >= 1,
        beta >= 0, alpha - beta == 1; one of the two may be omitted and is inferred.  (1, 0), the default, is LRPSequentialPresetA's
        alpha1beta0; (2, 1) is LRPAlpha2Beta1 / LRPSequentialPresetB.  A change drops the encode caches: call encode_images
        again.  beta > 0 on a ResNet encoder needs a stem width and stack widths that are multiples of 8 (ResNet-50/101/152 are;
        NotImplementedError otherwise) and runs in 'bf16x3' and 'fp32'; it is not built for the 'f16x2' walk of the VGG-style
        encoder (the explain calls raise NotImplementedError there)."""
        from .analyzer import infer_alpha_beta
        alpha, beta = infer_alpha_beta(alpha, beta, "LRPEngine.set_cnn_rule")
        _capi.check(self._lib.lrp_set_cnn_rule(self._h, float(alpha), float(beta)))
        if (alpha, beta) != self.cnn_rule:
            self.n_images = 0                            # the library dropped the caches of the other rule
            self.captions = None
        self.cnn_rule = (alpha, beta)
        self.cnn_rules = None                           # (the one rule replaces a table: set_cnn_rules)

    @staticmethod
    def _fill_rule(rec, r):
        """a record of analyzer.normalize_rule -> lrp_conv_rule"""
        if r[0] == "alphabeta":
            rec.kind, rec.alpha, rec.beta, rec.bias = _capi.LRP_RULE_ALPHA_BETA, r[1], r[2], int(r[3])
        elif r[0] == "epsilon":
            rec.kind, rec.eps, rec.bias = _capi.LRP_RULE_EPSILON, r[1], int(r[2])
        elif r[0] == "bounded":
            rec.kind, rec.low, rec.high = _capi.LRP_RULE_BOUNDED, r[1], r[2]
        else:
            rec.kind = _capi.LRP_RULE_FLAT if r[0] == "flat" else _capi.LRP_RULE_WSQUARE

    def set_cnn_rules(self, table):
        """One rule per conv of the VGG-style encoder's LRP walk (lrp_set_cnn_rules), input layer first.  `table`: a list with one
        entry per conv — ("alphabeta", alpha, beta, bias), ("epsilon", eps, bias), ("flat",), ("wsquare",), ("bounded", low, high)
        (the last three at the input layer only) — or anything analyzer.rule_table() accepts with this engine's conv count.
        The same alpha-beta rule with bias on every conv is set_cnn_rule(alpha, beta).  A change drops the encode caches: call
        encode_images again.  Epsilon kinds need set_precision('fp32') (the explain calls raise NotImplementedError otherwise)."""
        from .analyzer import normalize_rule
        table = tuple(normalize_rule(r) for r in table)
        arr = (_capi.LrpConvRule * max(1, len(table)))()
        for rec, r in zip(arr, table):
            self._fill_rule(rec, r)
        _capi.check(self._lib.lrp_set_cnn_rules(self._h, C.cast(arr, C.c_void_p), len(table)))
        uniform = table[0][0] == "alphabeta" and table[0][3] and all(r == table[0] for r in table)
        new_rule, new_table = ((table[0][1], table[0][2]), None) if uniform else (None, table)
        if (new_rule, new_table) != (self.cnn_rule, getattr(self, "cnn_rules", None)):
            self.n_images = 0                            # the library dropped the caches of the other rules
            self.captions = None
        self.cnn_rule, self.cnn_rules = new_rule, new_table

    def set_resnet_rules(self, rule, input_layer_rule=None):
        """The rule pair of the ResNet encoder's LRP walk (lrp_set_resnet_rules): `rule` for every conv above the stem —
        ("alphabeta", alpha, beta, bias) or ("epsilon", eps, bias) — and `input_layer_rule` for the stem conv — those, ("flat",),
        ("wsquare",), ("bounded", low, high) or (low, high); None: `rule` there too.  Records as analyzer.normalize_rule returns
        them, or anything it accepts.  The same alpha-beta rule with bias in both places is set_cnn_rule(alpha, beta).  A change
        drops the encode caches: call encode_images again.  Epsilon kinds need set_precision('fp32') (the explain calls raise
        NotImplementedError otherwise); beta > 0 needs widths that are multiples of 8, as set_cnn_rule."""
        from .analyzer import resnet_rule_pair
        stem, units = resnet_rule_pair(rule, input_layer_rule)
        arr = (_capi.LrpConvRule * 2)()
        for rec, r in zip(arr, (stem, units)):
            self._fill_rule(rec, r)
        _capi.check(self._lib.lrp_set_resnet_rules(self._h, C.addressof(arr[0]), C.addressof(arr[1])))
        uniform = stem == units and stem[0] == "alphabeta" and stem[3]
        new_rule, new_table = ((stem[1], stem[2]), None) if uniform else (None, (stem, units))
        if (new_rule, new_table) != (self.cnn_rule, getattr(self, "cnn_rules", None)):
            self.n_images = 0                            # the library dropped the caches of the other pair
            self.captions = None
        self.cnn_rule, self.cnn_rules = new_rule, new_table

    def set_deeplift_reference(self, reference=0, approximate_gradient=True):
        """The reference of the DeepLIFT walk (lrp_set_deeplift_reference; cnn_walk(..., 'deeplift')): a scalar, or an array that
        broadcasts to (1, H, W, 3) as the reference's reference_inputs does — one reference for all images.
        approximate_gradient: True (the per-element switch to the gradient where |x - reference| < 1e-7), False, or None to take
        the reference away again.  VGG-style encoders in 'fp32' mode only (NotImplementedError from this call on a ResNet engine,
        from the walk in the other modes).  A change drops the encode caches: call encode_images again."""
        H, W = self.img_hw
        if approximate_gradient is None:
            mode, ref = 0, None
        else:
            mode = 2 if approximate_gradient else 1
            ref = np.asarray(reference.detach().cpu() if torch.is_tensor(reference) else reference, dtype=np.float32)
        key = None if mode == 0 else (mode, ref.tobytes(), ref.shape)
        if mode == 0 or ref.ndim == 0:
            arr, scalar = None, float(ref) if mode else 0.0
        else:
            arr = np.ascontiguousarray(np.broadcast_to(ref, (1, H, W, 3)), dtype=np.float32)
            scalar = 0.0
        _capi.check(self._lib.lrp_set_deeplift_reference(self._h, arr.ctypes.data_as(C.c_void_p) if arr is not None else None,
                                                         scalar, mode))
        if key != getattr(self, "_deeplift_key", None):
            self.n_images = 0                            # the library dropped the caches of the other reference
            self.captions = None
        self._deeplift_key = key

    # ------------------------------------------------------------------ PatternNet / PatternAttribution
    PATTERN_TYPES = {"linear": _capi.LRP_PATTERN_LINEAR, "relu": _capi.LRP_PATTERN_RELU_POSITIVE,
                     "relu.positive": _capi.LRP_PATTERN_RELU_POSITIVE, "relu.negative": _capi.LRP_PATTERN_RELU_NEGATIVE}

    def _pattern_shapes(self):
        return [(3, 3, int(cin), int(cout)) for _, cin, cout, _ in self.cnn_cfg]

    def pattern_fit(self, images, pattern_type="relu", batch=None):
        """Fit the patterns of every conv on `images` (B, H, W, 3) (tools/pattern.py:220-336; lrp_pattern_fit_*): the images are
        encoded in batches of at most `batch` (default max_images) and accumulated on the device, then the patterns are computed
        and installed.  pattern_type: 'linear', 'relu' (= 'relu.positive') or 'relu.negative'.  Returns get_patterns().
        VGG-style engines in 'fp32' mode only.  The encode caches afterwards belong to the last batch."""
        if pattern_type not in self.PATTERN_TYPES:
            raise ValueError("unknown pattern type %r: one of %s" % (pattern_type, sorted(self.PATTERN_TYPES)))
        x = self._dev(images)
        if x.dim() != 4 or tuple(x.shape[1:]) != (self.img_hw[0], self.img_hw[1], 3):
            raise ValueError("images must be (B,%d,%d,3)" % self.img_hw)
        step = min(self.max_images, int(batch) if batch else self.max_images)
        if step < 1 or x.shape[0] < 1:
            raise ValueError("pattern_fit needs at least one image and a batch of at least 1")
        self.pattern_fit_begin(pattern_type)
        for lo in range(0, int(x.shape[0]), step):
            self.encode_images(x[lo:lo + step])
            self.pattern_fit_batch()
        self.pattern_fit_end()
        return self.get_patterns()

    def pattern_fit_begin(self, pattern_type="relu"):
        """Open a fit (lrp_pattern_fit_begin): zeroes the sums and drops the encode caches; then encode_images +
        pattern_fit_batch per batch, pattern_fit_end to install the patterns."""
        if pattern_type not in self.PATTERN_TYPES:
            raise ValueError("unknown pattern type %r: one of %s" % (pattern_type, sorted(self.PATTERN_TYPES)))
        _capi.check(self._lib.lrp_pattern_fit_begin(self._h, self.PATTERN_TYPES[pattern_type]))
        self.n_images = 0
        self.captions = None

    def pattern_fit_batch(self):
        _capi.check(self._lib.lrp_pattern_fit_batch(self._h, self._stream()))

    def pattern_fit_end(self):
        _capi.check(self._lib.lrp_pattern_fit_end(self._h, self._stream()))

    def pattern_stats(self):
        """The fit's float64 sums per conv (lrp_pattern_stats): a list of dicts with Sx, Sxy (3, 3, cin, cout), cnt, Sy (cout,)
        and P (a float), as numpy arrays."""
        out = []
        for li, (_, _, cin, cout) in enumerate(self._pattern_shapes()):
            kc = 9 * cin * cout
            buf = torch.empty((2 * kc + 2 * cout + 1,), dtype=torch.float64, device=self.device)
            _capi.check(self._lib.lrp_pattern_stats(self._h, li, C.c_void_p(buf.data_ptr()), buf.numel(), self._stream()))
            b = buf.cpu().numpy()
            out.append({"Sx": b[:kc].reshape(3, 3, cin, cout), "Sxy": b[kc:2 * kc].reshape(3, 3, cin, cout),
                        "cnt": b[2 * kc:2 * kc + cout], "Sy": b[2 * kc + cout:2 * kc + 2 * cout], "P": float(b[-1])})
        return out

    def set_patterns(self, patterns):
        """One (3, 3, cin, cout) array per conv (lrp_set_patterns): what the 'patternnet' / 'pattern_attribution' walks run on."""
        shapes = self._pattern_shapes()
        patterns = list(patterns)
        if len(patterns) != len(shapes):
            raise ValueError("one pattern per conv: %d given, %d convs" % (len(patterns), len(shapes)))
        for li, (p, shp) in enumerate(zip(patterns, shapes)):
            t = self._dev(p)
            if tuple(t.shape) != shp:
                raise ValueError("pattern %d: expected HWIO %s, got %s" % (li, shp, tuple(t.shape)))
            _capi.check(self._lib.lrp_set_patterns(self._h, li, C.c_void_p(t.data_ptr()), self._stream()))

    def get_patterns(self):
        """The patterns the engine holds, fitted or set: a list of (3, 3, cin, cout) float32 numpy arrays (lrp_get_patterns)."""
        out = []
        for li, shp in enumerate(self._pattern_shapes()):
            t = torch.empty(shp, dtype=torch.float32, device=self.device)
            _capi.check(self._lib.lrp_get_patterns(self._h, li, C.c_void_p(t.data_ptr()), self._stream()))
            out.append(t.cpu().numpy())
        return out

    def set_pattern_projection(self, on):
        """reverse_project_bottleneck_layers of the pattern walks (lrp_set_pattern_projection; default on): every reversed tensor
        is divided per row by its absolute maximum before it is used."""
        _capi.check(self._lib.lrp_set_pattern_projection(self._h, int(bool(on))))
        self.pattern_projection = bool(on)

    def set_fast_layers(self, mask):
        """Which conv layers take the two-MFMA form in 'f16x2' mode (lrp_set_fast_layers): bit li of `mask`, an iterable of
        layer indices, or None / -1 for the built-in rule.  0 = fp16 pairs with three MFMAs in every layer.  A change drops
        the encode caches while the engine is in 'f16x2' mode.  See calibration.calibrate_fast_mode for a measured choice."""
        if mask is None:
            mask = -1
        elif not isinstance(mask, int):
            mask = sum(1 << int(li) for li in set(mask))
        _capi.check(self._lib.lrp_set_fast_layers(self._h, int(mask)))
        if self.precision == "f16x2" and mask != getattr(self, "fast_layers", -1):
            self.n_images = 0
            self.captions = None
        self.fast_layers = mask

    # ------------------------------------------------------------------ profiling hooks (bench.py)
    def profile_enable(self, on=True):
        _capi.check(self._lib.lrp_profile_enable(self._h, int(bool(on))))

    def profile_query(self):
        n, ms, fl = C.c_int64(), C.c_double(), C.c_double()
        _capi.check(self._lib.lrp_profile_query(self._h, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value


def _profile_records(self, cap=256):
    ms = (C.c_double * cap)()
    fl = (C.c_double * cap)()
    n = C.c_int32()
    _capi.check(self._lib.lrp_profile_records(self._h, cap, ms, fl, C.byref(n)))
    return [(ms[i], fl[i]) for i in range(n.value)]


LRPEngine.profile_records = _profile_records


CONV_SPLIT_BF16 = 0x100
CONV_WREG = 0x200


def op_conv(x, w_hwio, bias, aux, mode, taps=9, split_bf16=False, wreg=False):
    """Operator-level entry for unit tests of the MFMA conv kernel (see lrp_op_conv); split_bf16 runs the
    same operator on the split-bf16 path (LRP_CONV_SPLIT_BF16), wreg with the fragment-major weight copy (LRP_CONV_WREG)."""
    lib = _capi.load()
    dev = x.device
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    Cin, Cout = w.shape[2], w.shape[3]
    NB, H, W, _ = x.shape
    bwd = mode >= 2
    if mode == 3:
        out = torch.empty((NB, 2 * H, 2 * W, Cin), dtype=torch.float32, device=dev)
    elif bwd:
        out = torch.empty((NB, H, W, Cin), dtype=torch.float32, device=dev)
    else:
        out = torch.empty((NB, H, W, Cout), dtype=torch.float32, device=dev)
    b = np.ascontiguousarray(bias, dtype=np.float32) if bias is not None else None
    _capi.check(lib.lrp_op_conv(C.c_void_p(x.data_ptr()), w.ctypes.data_as(C.c_void_p),
                                b.ctypes.data_as(C.c_void_p) if b is not None else None,
                                C.c_void_p(aux.data_ptr()) if aux is not None else None,
                                C.c_void_p(out.data_ptr()), NB, H, W, Cin, Cout, taps,
                                mode | (CONV_SPLIT_BF16 if split_bf16 else 0) | (CONV_WREG if wreg else 0),
                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out


def op_conv_ab(sp, sn, w_hwio, alpha, beta, gp, gn, pool=False, split_bf16=False):
    """The two-chain launch of the alpha-beta walk (lrp_op_conv_ab): c = convT(sp, alpha w+) + convT(sn, -beta w-) in one GEMM,
    outputs (c x gp, c x gn), c repeated 2 x 2 with pool.  sp, sn (NB, H, W, Cout) float32 device tensors, w_hwio (3, 3, Cin,
    Cout) numpy, gp, gn (NB, H u, W u, Cin)."""
    lib = _capi.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    Cin, Cout = w.shape[2], w.shape[3]
    NB, H, W, _ = sp.shape
    u = 2 if pool else 1
    assert tuple(sn.shape) == (NB, H, W, Cout) == tuple(sp.shape)
    assert tuple(gp.shape) == tuple(gn.shape) == (NB, u * H, u * W, Cin)
    sp, sn, gp, gn = sp.contiguous(), sn.contiguous(), gp.contiguous(), gn.contiguous()
    outp = torch.empty((NB, u * H, u * W, Cin), dtype=torch.float32, device=sp.device)
    outn = torch.empty_like(outp)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_conv_ab(p(sp), p(sn), w.ctypes.data_as(C.c_void_p), float(alpha), float(beta), p(gp), p(gn), p(outp), p(outn),
                                   NB, H, W, Cin, Cout, int(bool(pool)), int(bool(split_bf16)), _cur_stream(sp.device)))
    return outp, outn


def op_conv_rule(chains, w_hwio, coef, gates, pool=False, split_bf16=False):
    """A launch of the rule table's walk (lrp_op_conv_rule): c = sum_j convT(chains[j], p_j w+ + q_j w-) in one GEMM, outputs
    [c x g for g in gates], c repeated 2 x 2 with pool.  chains: one or two (NB, H, W, Cout) float32 device tensors, coef: a
    (p, q) per chain, gates: one or two (NB, H u, W u, Cin) tensors; w_hwio (3, 3, Cin, Cout) numpy."""
    lib = _capi.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    Cin, Cout = w.shape[2], w.shape[3]
    chains = [t.contiguous() for t in chains]
    gates = [t.contiguous() for t in gates]
    NB, H, W, _ = chains[0].shape
    u = 2 if pool else 1
    assert len(chains) in (1, 2) and len(gates) in (1, 2) and len(coef) == len(chains)
    assert all(tuple(t.shape) == (NB, H, W, Cout) for t in chains) and all(tuple(t.shape) == (NB, u * H, u * W, Cin) for t in gates)
    outs = [torch.empty((NB, u * H, u * W, Cin), dtype=torch.float32, device=chains[0].device) for _ in gates]
    p = lambda t: C.c_void_p(t.data_ptr())
    opt = lambda ts, i: p(ts[i]) if len(ts) > i else None
    pq = [float(v) for c in coef for v in c] + [0.0, 0.0]
    _capi.check(lib.lrp_op_conv_rule(p(chains[0]), opt(chains, 1), w.ctypes.data_as(C.c_void_p), len(chains), len(gates), pq[0], pq[1],
                                     pq[2], pq[3], p(gates[0]), opt(gates, 1), p(outs[0]), opt(outs, 1), NB, H, W, Cin, Cout,
                                     int(bool(pool)), int(bool(split_bf16)), _cur_stream(chains[0].device)))
    return outs


def op_deeplift_conv(x, xr, a, w_hwio, bias, pool=False, approximate_gradient=True):
    """One fused conv + ReLU layer of the DeepLIFT walk (lrp_op_deeplift_conv), exact fp32: x (NB, H, W, Cin) and the shared reference
    input xr (H, W, Cin) go through the layer, the incoming a (NB, H u, W u, Cout), u = 1/2 with pool, is routed to the arg-max of
    the image's activation and mapped back with LinearRule; returns (NB, H, W, Cin).  Cin is 3 or a multiple of 4."""
    lib = _capi.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    b = np.ascontiguousarray(bias, dtype=np.float32)
    Cin, Cout = w.shape[2], w.shape[3]
    NB, H, W, _ = x.shape
    d = 2 if pool else 1
    assert tuple(x.shape) == (NB, H, W, Cin) and tuple(xr.shape) == (H, W, Cin) and tuple(a.shape) == (NB, H // d, W // d, Cout)
    x, xr, a = x.contiguous(), xr.contiguous(), a.contiguous()
    out = torch.empty((NB, H, W, Cin), dtype=torch.float32, device=x.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_deeplift_conv(p(x), p(xr), p(a), w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), p(out), NB, H, W,
                                         Cin, Cout, int(bool(pool)), 2 if approximate_gradient else 1, _cur_stream(x.device)))
    return out


def op_conv_pool_sparse(sc, pos, w_hwio, gate, reps=1):
    """The conv-LRP launch behind a 2x2 max-pool on the 2:4-sparse matrix cores (lrp_op_conv_pool_sparse): sc (NB, Hp, Wp, Cout)
    float32 = each window's one non-zero, pos (same shape) uint8 = its position 2 dy + dx, w_hwio (3, 3, Cin, Cout) numpy,
    gate (NB, 2 Hp, 2 Wp, Cin) -> (NB, 2 Hp, 2 Wp, Cin) float32."""
    lib = _capi.load()
    w = np.ascontiguousarray(w_hwio, dtype=np.float32)
    Cin, Cout = w.shape[2], w.shape[3]
    NB, Hp, Wp, _ = sc.shape
    assert pos.dtype == torch.uint8 and tuple(pos.shape) == tuple(sc.shape) and tuple(gate.shape) == (NB, 2 * Hp, 2 * Wp, Cin)
    sc, pos, gate = sc.contiguous(), pos.contiguous(), gate.contiguous()
    out = torch.empty((NB, 2 * Hp, 2 * Wp, Cin), dtype=torch.float32, device=sc.device)
    _capi.check(lib.lrp_op_conv_pool_sparse(C.c_void_p(sc.data_ptr()), C.c_void_p(pos.data_ptr()), w.ctypes.data_as(C.c_void_p),
                                            C.c_void_p(gate.data_ptr()), C.c_void_p(out.data_ptr()), NB, Hp, Wp, Cin, Cout, int(reps),
                                            _cur_stream(sc.device)))
    return out


def op_sgemm(A, B, transA=False, transB=False, C_init=None, split=True):
    """C (+)= op(A) op(B) through lrp_op_sgemm (fp32 MFMA); A, B 2-D device tensors (views with a row stride allowed)."""
    lib = _capi.load()
    M, K = (A.shape[1], A.shape[0]) if transA else A.shape
    N = B.shape[0] if transB else B.shape[1]
    out = torch.empty((M, N), dtype=torch.float32, device=A.device) if C_init is None else C_init
    ws = torch.empty(8 << 20, dtype=torch.float32, device=A.device) if split else None
    _capi.check(lib.lrp_op_sgemm(C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(out.data_ptr()), M, N, K,
                                 A.stride(0), B.stride(0), out.stride(0), int(transA), int(transB), int(C_init is not None),
                                 C.c_void_p(ws.data_ptr()) if ws is not None else None, ws.numel() if ws is not None else 0,
                                 _cur_stream(A.device)))
    return out


def op_conv_wgrad(x, dz, bf16=False):
    """Weight / bias gradient of a 3x3 'same' conv (lrp_op_conv_wgrad[_bf16]): x (NB,H,W,Cin), dz (NB,H,W,Cout) -> (dw HWIO, db)."""
    lib = _capi.load()
    NB, H, W, Cin = x.shape
    Cout = dz.shape[3]
    dw = torch.empty((3, 3, Cin, Cout), dtype=torch.float32, device=x.device)
    db = torch.empty((Cout,), dtype=torch.float32, device=x.device)
    ws = torch.empty(16 << 20, dtype=torch.float32, device=x.device)
    fn = lib.lrp_op_conv_wgrad_bf16 if bf16 else lib.lrp_op_conv_wgrad
    _capi.check(fn(C.c_void_p(x.data_ptr()), C.c_void_p(dz.data_ptr()), C.c_void_p(dw.data_ptr()),
                                      C.c_void_p(db.data_ptr()), NB, H, W, Cin, Cout, C.c_void_p(ws.data_ptr()), ws.numel(),
                                      _cur_stream(x.device)))
    return dw, db


def _cur_stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def op_epsilon_dense(x, W, R, epsilon):
    """EpsilonRule(bias=False) for a Dense layer (RR:113-144): x (N,Din), W (Din,Dout) numpy, R (N,Dout)."""
    lib = _capi.load()
    W = np.ascontiguousarray(W, dtype=np.float32)
    out = torch.empty_like(x)
    _capi.check(lib.lrp_op_epsilon_dense(C.c_void_p(x.data_ptr()), W.ctypes.data_as(C.c_void_p), C.c_void_p(R.data_ptr()),
                                         C.c_void_p(out.data_ptr()), x.shape[0], W.shape[0], W.shape[1], float(epsilon),
                                         _cur_stream(x.device)))
    return out


def op_batchnorm_lrp(x, gamma, beta, mean, var, bn_eps, R):
    """BatchNormalizationReverseLayer (RA:197-257), channels-last tensors on the GPU."""
    lib = _capi.load()
    out = torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_batchnorm_lrp(p(x), p(gamma), p(beta), p(mean), p(var), float(bn_eps), p(R), p(out), x.numel(),
                                         x.shape[-1], _cur_stream(x.device)))
    return out


def op_add_lrp(a, b, R):
    """AddReverseLayer (RA:260-286)."""
    lib = _capi.load()
    Ra, Rb = torch.empty_like(a), torch.empty_like(b)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_add_lrp(p(a), p(b), p(R), p(Ra), p(Rb), a.numel(), _cur_stream(a.device)))
    return Ra, Rb


def op_avgpool_lrp(x, R, k):
    """AveragePoolingReverseLayer (RA:289-316), k x k / stride k average pooling, channels-last."""
    lib = _capi.load()
    x, R = x.contiguous(), R.contiguous()
    NB, H, W, Cc = x.shape
    out = torch.empty_like(x)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_avgpool_lrp(p(x), p(R), p(out), NB, H, W, Cc, int(k), _cur_stream(x.device)))
    return out


def log_softmax_topk(logits, k):
    """lrp_op_log_softmax_topk: logits (rows, V) float64 device tensor -> (ids int32 (rows, k), logp float64 (rows, k))."""
    lib = _capi.load()
    x = logits.contiguous()
    if x.dtype != torch.float64 or x.dim() != 2:
        raise ValueError("expected a (rows, V) float64 tensor")
    rows, V = x.shape
    ids = torch.empty((rows, k), dtype=torch.int32, device=x.device)
    lp = torch.empty((rows, k), dtype=torch.float64, device=x.device)
    _capi.check(lib.lrp_op_log_softmax_topk(C.c_void_p(x.data_ptr()), rows, V, int(k), C.c_void_p(ids.data_ptr()),
                                            C.c_void_p(lp.data_ptr()), _cur_stream(x.device)))
    return ids, lp


def _beam_result_views(n, k, max_len, device, buf=None):
    """The four results of a search as views of one byte buffer (so that they reach the host in one copy):
    logp (n, k) float64 | captions (n, k, max_len + 1) int32 | lengths (n, k) int32 | n_complete (n,) int32."""
    sizes = [n * k * 8, n * k * (max_len + 1) * 4, n * k * 4, n * 4]
    if buf is None:
        buf = torch.empty(sum(sizes), dtype=torch.uint8, device=device)
    o = [0, sizes[0], sizes[0] + sizes[1], sizes[0] + sizes[1] + sizes[2], sum(sizes)]
    logp = buf[o[0]:o[1]].view(torch.float64).view(n, k)
    caps = buf[o[1]:o[2]].view(torch.int32).view(n, k, max_len + 1)
    lens = buf[o[2]:o[3]].view(torch.int32).view(n, k)
    ncomp = buf[o[3]:o[4]].view(torch.int32)
    return buf, (caps, lens, logp, ncomp)


def beam_lists(captions, lengths):
    """(n, k, max_len + 1) captions and (n, k) lengths -> per image the list of captions `beam.search` returns."""
    caps, lens = captions.cpu().numpy(), lengths.cpu().numpy()
    return [[caps[i, q, :lens[i, q]].tolist() for q in range(caps.shape[1]) if lens[i, q] > 0] for i in range(caps.shape[0])]


def beam_state(n_images, k, max_len, device):
    """An (uninitialised) state buffer for `beam_select` / `beam_finish`: lrp_op_beam_state_bytes bytes on `device`."""
    nbytes = _capi.load().lrp_op_beam_state_bytes(int(n_images), int(k), int(max_len))
    if nbytes < 0:
        raise ValueError("need n_images >= 1, max_len >= 1 and 1 <= k <= 32")
    return torch.empty(nbytes // 8, dtype=torch.int64, device=device)


def beam_select(state, ids, logp, step, eos, max_len):
    """lrp_op_beam_select: search step `step` of the beam bookkeeping (explainers.py:51-120, as `beam.search` restates it) for
    all images at once.  state = `beam_state(n_images, k, max_len, device)`; ids (n_images * k, k) int32 model columns and logp
    (n_images * k, k) float64 as `log_softmax_topk` returns them.  Returns (parent, word), (n_images * k,) int32 device tensors:
    row r of the next step continues row parent[r] with tokenizer id word[r]."""
    lib = _capi.load()
    ids, logp = ids.contiguous(), logp.contiguous()
    if ids.dtype != torch.int32 or logp.dtype != torch.float64 or ids.dim() != 2 or ids.shape != logp.shape:
        raise ValueError("expected ids int32 and logp float64 of one (n_images * k, k) shape")
    rows, k = ids.shape
    if k < 1 or rows % k:
        raise ValueError("ids must have n_images * k rows of k columns")
    n = rows // k
    if state.numel() * state.element_size() < lib.lrp_op_beam_state_bytes(n, k, int(max_len)):
        raise ValueError("state is smaller than lrp_op_beam_state_bytes(n_images, k, max_len)")
    parent = torch.empty(rows, dtype=torch.int32, device=ids.device)
    word = torch.empty(rows, dtype=torch.int32, device=ids.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_beam_select(p(state), p(ids), p(logp), n, k, int(max_len), int(step), int(eos), p(parent), p(word),
                                       _cur_stream(ids.device)))
    return parent, word


def beam_finish(state, n_images, k, max_len, steps, eos):
    """lrp_op_beam_finish after `steps` calls of `beam_select`: (captions (n_images, k, max_len + 1) int32 with a trailing EOS,
    lengths (n_images, k) int32, logp (n_images, k) float64, n_complete (n_images,) int32) — `LRPEngine.beam_search`'s results."""
    lib = _capi.load()
    n, k = int(n_images), int(k)
    if n < 1 or k < 1 or state.numel() * state.element_size() < lib.lrp_op_beam_state_bytes(n, k, int(max_len)):
        raise ValueError("state is smaller than lrp_op_beam_state_bytes(n_images, k, max_len)")
    _, views = _beam_result_views(n, k, int(max_len), state.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    _capi.check(lib.lrp_op_beam_finish(p(state), n, k, int(max_len), int(steps), int(eos), p(views[0]), p(views[1]), p(views[2]),
                                       p(views[3]), _cur_stream(state.device)))
    return views


_LUT_CACHE = {}


def heatmap_render(R_img, gamma=0.95, color_conversion=None):
    """`heatmap(postprocess(relevance, color_conversion))` of the harness (explain_image.py:55-60) on the device:
    R_img (n, H, W, 3) relevance tensor -> (n, H, W, 3) float32 RGB in [0, 1] (seismic colormap)."""
    from .postprocess import _seismic
    lib = _capi.load()
    R = R_img.contiguous()
    if color_conversion in ("RGBtoBGR", "BGRtoRGB"):
        R = R.flip(-1).contiguous()              # (the channel sum does not care, the gamma maximum neither)
    n, Hh, Ww, Cc = R.shape
    key = str(R.device)
    if key not in _LUT_CACHE:
        _LUT_CACHE[key] = torch.as_tensor(np.ascontiguousarray(_seismic(np.arange(256)), dtype=np.float32)).to(R.device)
    out = torch.empty((n, Hh, Ww, 3), dtype=torch.float32, device=R.device)
    _capi.check(lib.lrp_heatmap_render(C.c_void_p(R.data_ptr()), C.c_void_p(_LUT_CACHE[key].data_ptr()),
                                       C.c_void_p(out.data_ptr()), n, Hh * Ww, Cc, C.c_float(gamma), _cur_stream(R.device)))
    return out


class switches(object):
    """`with switches(LRP_UP2_PW=0, ...):` — set the library's A/B switches for the body and restore the
    environment afterwards (lrp_reload_switches re-reads them: they are not looked up on the launch path).  For tests and
    measurement scripts; a switch that changes the encode caches takes effect at the next encode_images."""

    def __init__(self, **env):
        self.env = {k: str(v) for k, v in env.items()}
        self.old = {}

    def __enter__(self):
        import os
        for k, v in self.env.items():
            if not k.startswith("LRP_"):
                raise ValueError("not a library switch: %s" % k)
            self.old[k] = os.environ.get(k)
            os.environ[k] = v
        _capi.check(_capi.load().lrp_reload_switches())
        return self

    def __exit__(self, *exc):
        import os
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _capi.check(_capi.load().lrp_reload_switches())
        return False


PLAN_FIELDS = ("ok", "form", "BM", "BN", "threads", "tw", "th", "hrows", "tpt", "m_tiles", "n_tiles")


def conv_plan(epi, prec, NB, H, W, N, Cin, taps=9, terms=7, split=0, flags=0):
    """lrp_conv_plan (ABI v8): the form of the implicit-GEMM convolution kernel this launch would take under the current
    switches, as a dict of PLAN_FIELDS.  Host arithmetic only: works without a GPU."""
    out = (C.c_int32 * len(PLAN_FIELDS))()
    _capi.check(_capi.load().lrp_conv_plan(epi, prec, terms, NB, H, W, N, Cin, taps, split, flags, out))
    return dict(zip(PLAN_FIELDS, out))


def preprocess_images(rgb_u8, size=(224, 224)):
    """models/preprocessors.py:38-53 on the device: (NB, H0, W0, 3) uint8 RGB tensor -> (NB, H, W, 3) float32 BGR,
    mean-subtracted, nearest-neighbour resized like keras `load_img(target_size=size)`."""
    lib = _capi.load()
    x = rgb_u8.contiguous()
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
        raise ValueError("expected a (NB, H0, W0, 3) uint8 tensor")
    NB, H0, W0, _ = x.shape
    out = torch.empty((NB, size[0], size[1], 3), dtype=torch.float32, device=x.device)
    _capi.check(lib.lrp_preprocess_images(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), NB, H0, W0, size[0], size[1],
                                          _cur_stream(x.device)))
    return out


def heatmap_scores(R_img, mode):
    """LRP-inference score per heat-map (model.py:1675-1686) on the device: R_img (n,H,W,C) -> (n,) float64."""
    lib = _capi.load()
    m = {"mean": 0, "pos_mean": 1, "quantile": 2}.get(mode)
    if m is None:
        raise NotImplementedError("the lrp inference mode is not available")
    R = R_img.contiguous()
    n, C_ = R.shape[0], R.shape[-1]
    out = torch.empty((n,), dtype=torch.float64, device=R.device)
    _capi.check(lib.lrp_heatmap_scores(C.c_void_p(R.data_ptr()), C.c_void_p(out.data_ptr()), n, R[0].numel() // C_, C_, m,
                                       _cur_stream(R.device)))
    return out


# ---- bounding-box correctness evaluation (evaluate_bbox.py; csrc/eval_kernels.h, lrp_eval_*)
def eval_relevance_maps(R_img, sign=-1):
    """`project(mean(max(sign * postprocess(R, 'BGRtoRGB'), 0), -1))` of the evaluator (evaluate_bbox.py:59-86) on the
    device: R_img (n, H, W, C) float32 or float64 tensor -> (n, H, W) maps of the same dtype, bit-identical to numpy."""
    lib = _capi.load()
    R = R_img.contiguous()
    if R.dtype not in (torch.float32, torch.float64) or R.dim() != 4:
        raise ValueError("expected an (n, H, W, C) float32 or float64 tensor")
    n, Hh, Ww, Cc = R.shape
    out = torch.empty((n, Hh, Ww), dtype=R.dtype, device=R.device)
    _capi.check(lib.lrp_eval_relevance_maps(C.c_void_p(R.data_ptr()), C.c_void_p(out.data_ptr()), int(R.dtype == torch.float64),
                                            n, Hh * Ww, Cc, int(sign), _cur_stream(R.device)))
    return out


def eval_expand_matrix(g, upscale, sigma=20.0):
    """(g * upscale, g) float64 M with pyramid_expand(A, upscale, sigma) = M A M^T (host only)."""
    lib = _capi.load()
    M = np.empty((g * upscale, g), dtype=np.float64)
    _capi.check(lib.lrp_eval_expand_matrix(int(g), int(upscale), float(sigma), M.ctypes.data_as(C.c_void_p)))
    return M


_EXPAND_CACHE = {}


def eval_attention_maps(att, g, upscale, sigma=20.0):
    """`project(pyramid_expand(att.reshape(g, g), upscale, sigma))` (evaluate_bbox.py:75-84) on the device:
    att (n, g * g) float32 tensor -> (n, S, S) float64, S = g * upscale."""
    lib = _capi.load()
    a = att.contiguous()
    if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != g * g:
        raise ValueError("expected an (n, g * g) float32 tensor")
    key = (str(a.device), int(g), int(upscale), float(sigma))
    if key not in _EXPAND_CACHE:
        _EXPAND_CACHE[key] = torch.as_tensor(eval_expand_matrix(g, upscale, sigma)).to(a.device)
    S = g * upscale
    out = torch.empty((a.shape[0], S, S), dtype=torch.float64, device=a.device)
    _capi.check(lib.lrp_eval_attention_maps(C.c_void_p(a.data_ptr()), C.c_void_p(_EXPAND_CACHE[key].data_ptr()),
                                            C.c_void_p(out.data_ptr()), a.shape[0], int(g), int(upscale), _cur_stream(a.device)))
    return out


def eval_box_scores(maps, boxes, thr):
    """Box scores of evaluate_bbox.py:191-208 on the device: maps (n, h, w) float32 / float64 tensor, boxes (nb, 5) int32
    (map, y0, y1, x0, x1), thr (nb, K) float64 (numpy or tensors) -> (nb, K) float64 tensor."""
    lib = _capi.load()
    m = maps.contiguous()
    if m.dtype not in (torch.float32, torch.float64) or m.dim() != 3:
        raise ValueError("expected an (n, h, w) float32 or float64 tensor")
    b = torch.as_tensor(np.asarray(boxes, dtype=np.int32) if not torch.is_tensor(boxes) else boxes).to(m.device).contiguous()
    t = torch.as_tensor(np.asarray(thr, dtype=np.float64) if not torch.is_tensor(thr) else thr).to(m.device).contiguous()
    if b.dtype != torch.int32 or b.dim() != 2 or b.shape[1] != 5 or t.dtype != torch.float64 or t.dim() != 2 \
            or t.shape[0] != b.shape[0]:
        raise ValueError("boxes must be (nb, 5) int32 and thr (nb, K) float64")
    nb, K = t.shape
    out = torch.empty((nb, K), dtype=torch.float64, device=m.device)
    _capi.check(lib.lrp_eval_box_scores(C.c_void_p(m.data_ptr()), int(m.dtype == torch.float64), m.shape[0], m.shape[1],
                                        m.shape[2], C.c_void_p(b.data_ptr()), C.c_void_p(t.data_ptr()), nb, K,
                                        C.c_void_p(out.data_ptr()), _cur_stream(m.device)))
    return out


# ---- Grad-CAM and the word examination (exaimin_word.py; csrc/gradcam_kernels.h, lrp_op_gradcam / lrp_exam_maps)
def _expand_matrix_dev(device, g, upscale, sigma):
    key = (str(device), int(g), int(upscale), float(sigma))
    if key not in _EXPAND_CACHE:
        _EXPAND_CACHE[key] = torch.as_tensor(eval_expand_matrix(g, upscale, sigma)).to(device)
    return _EXPAND_CACHE[key]


def op_gradcam(feat, img_idx, grads, g, upscale, gb=None, sigma=20.0):
    """`grad_cam` (explainers.py:939-949) for n (image, word) units in fp64 on the device: feat (B, L, D) float32 tensor,
    img_idx n image indices, grads (n, L, D) float32 tensor, L = g * g -> cam (n, S, S) float64, S = g * upscale.
    With gb (n, S, S, C) float32 (the guided-backprop map) -> (gb * cam (n, S, S, C) float64, cam)."""
    lib = _capi.load()
    f, d = feat.contiguous(), grads.contiguous()
    if f.dtype != torch.float32 or d.dtype != torch.float32 or f.dim() != 3 or d.dim() != 3 or f.shape[1:] != d.shape[1:] \
            or f.shape[1] != g * g:
        raise ValueError("expected feat (B, g * g, D) and grads (n, g * g, D) float32 tensors")
    n, B, D, S = d.shape[0], f.shape[0], f.shape[2], g * upscale
    ii = np.asarray(img_idx.cpu() if torch.is_tensor(img_idx) else img_idx, dtype=np.int64).reshape(-1)
    if len(ii) != n or (n and (ii.min() < 0 or ii.max() >= B)):
        raise ValueError("img_idx must hold n indices in [0, %d)" % B)
    idx = torch.as_tensor(ii.astype(np.int32)).to(f.device)
    out = None
    if gb is not None:
        gb = gb.contiguous()
        if gb.dtype != torch.float32 or gb.dim() != 4 or tuple(gb.shape[:3]) != (n, S, S):
            raise ValueError("gb must be an (n, S, S, C) float32 tensor")
        out = torch.empty(gb.shape, dtype=torch.float64, device=f.device)
    M = _expand_matrix_dev(f.device, g, upscale, sigma)      # validates g, upscale and sigma
    cam = torch.empty((n, S, S), dtype=torch.float64, device=f.device)
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    _capi.check(lib.lrp_op_gradcam(p(f), p(idx), p(d), p(M), p(gb), p(cam), p(out), n, B, int(g), int(upscale), D,
                                   gb.shape[3] if gb is not None else 0, _cur_stream(f.device)))
    return cam if gb is None else (out, cam)


# ---- augment and reduce of SmoothGrad / IntegratedGradients (wrapper.py:78-345; csrc/augment_kernels.h)
_POST = {None: 0, "abs": 1, "square": 2}
_p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None


def _aug_input(x):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() < 2 or not x.is_cuda:
        raise ValueError("expected a (B, ...) float32 tensor on the device")
    x = x.contiguous()
    return x, int(x.shape[0]), int(x[0].numel())


def _aug_rows(B, n, r0, count):
    n, r0 = int(n), int(r0)
    count = B * n - r0 if count is None else int(count)
    if n < 1 or r0 < 0 or count < 1 or r0 + count > B * n:
        raise ValueError("rows [%d, %d) are not rows of the (%d * %d, per_image) sample matrix" % (r0, r0 + count, B, n))
    return n, r0, count


def _aug_ref(x, ref):
    """reference_inputs -> (tensor or None, scalar)"""
    if np.isscalar(ref):
        return None, float(ref)
    r = ref if torch.is_tensor(ref) else torch.as_tensor(np.ascontiguousarray(ref, dtype=np.float32))
    r = r.to(device=x.device, dtype=torch.float32)
    try:
        r = r.broadcast_to(x.shape).contiguous()
    except RuntimeError:
        raise ValueError("reference_inputs must be a scalar or broadcast to the input's shape %s" % (tuple(x.shape),))
    return r, 0.0


def op_augment_gaussian(x, n, sigma, seed=0, r0=0, count=None, out=None):
    """Rows [r0, r0 + count) of GaussianSmoother's sample matrix (wrapper.py:221-225 in np.repeat order: row b * n + s is
    x[b] + sigma * N(seed, row, element)) -> (count, ...) float32 tensor.  The noise is Philox4x32-10 + Box-Muller, a pure
    function of (seed, row, element) (include/lrp_hip.h): any chunking gives the same bits."""
    x, B, per = _aug_input(x)
    n, r0, count = _aug_rows(B, n, r0, count)
    if out is None:
        out = torch.empty((count,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _capi.check(_capi.load().lrp_op_augment_gaussian(_p(x), _p(out), B, n, per, r0, count, float(sigma),
                                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _cur_stream(x.device)))
    return out


def op_augment_path(x, n, reference=0, path="reference", r0=0, count=None, out=None):
    """Rows [r0, r0 + count) of PathIntegrator's sample matrix: path='reference' is what the reference computes,
    x + (s / n) (x - ref) (wrapper.py:268-288); path='standard' the published ref + (s / n) (x - ref)."""
    if path not in ("reference", "standard"):
        raise ValueError("path must be 'reference' or 'standard'")
    x, B, per = _aug_input(x)
    n, r0, count = _aug_rows(B, n, r0, count)
    rt, rs = _aug_ref(x, reference)
    if out is None:
        out = torch.empty((count,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _capi.check(_capi.load().lrp_op_augment_path(_p(x), _p(rt), rs, _p(out), B, n, per, r0, count,
                                                 0 if path == "reference" else 1, _cur_stream(x.device)))
    return out


def op_reduce_accumulate(maps, acc, n, r0=0, post=None):
    """acc (B, ...) float64 += the rows of a chunk: maps (count, ...) float32 holds the maps of samples [r0, r0 + count);
    post None / 'abs' / 'square' is applied per sample (gradient_based.py:110-137).  One thread per element, ascending
    sample order, launches in stream order: the sum does not depend on the chunking."""
    if post not in _POST:
        raise ValueError("Parameter 'postprocess' must be either None, 'abs', or 'square'.")
    if not torch.is_tensor(acc) or acc.dtype != torch.float64 or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous (B, ...) float64 tensor")
    m, count, per = _aug_input(maps)
    B = int(acc.shape[0])
    if int(acc[0].numel()) != per:
        raise ValueError("maps and acc differ in the size of a map")
    n, r0, count = _aug_rows(B, n, r0, count)
    _capi.check(_capi.load().lrp_op_reduce_mean(0, _p(m), _p(acc), B, n, per, r0, count, _POST[post], None, None, None, 0.0, 0,
                                                _cur_stream(m.device)))
    return acc


def op_reduce_finish(acc, n, x=None, reference=0, out=None):
    """float32(acc / n), or with x float32(acc / n * (x - reference)) (PathIntegrator, wrapper.py:290-296), rounded once."""
    if not torch.is_tensor(acc) or acc.dtype != torch.float64 or not acc.is_contiguous():
        raise ValueError("acc must be a contiguous (B, ...) float64 tensor")
    B, per = int(acc.shape[0]), int(acc[0].numel())
    rt, rs = None, 0.0
    if x is not None:
        x, Bx, perx = _aug_input(x)
        if (Bx, perx) != (B, per):
            raise ValueError("x and acc differ in shape")
        rt, rs = _aug_ref(x, reference)
    if out is None:
        out = torch.empty(acc.shape, dtype=torch.float32, device=acc.device)
    _capi.check(_capi.load().lrp_op_reduce_mean(1, None, _p(acc), B, int(n), per, 0, 0, 0, _p(out), _p(x), _p(rt), rs,
                                                0 if x is None else 1, _cur_stream(acc.device)))
    return out


_EXAM_POOL = {None: 0, "max": 1, "ave": 2}


def exam_maps(R_img, pool=None, k=None, absval=False, want_maps=True):
    """The map and statistic of the word examination (exaimin_word.py:95-102, :131-160, :488-489) on the device: R_img
    (n, H, W, C) float32 or float64 tensor -> channel mean (flipped channel order, input dtype), pool None / 'max' / 'ave'
    over k x k blocks, x / absmax, |x| if absval.  Returns (maps, means): maps (n, H, W) in the input dtype, or
    (n, H / k, W / k) float64 when pooled (None unless want_maps); means (n,) float64, the mean of each map."""
    lib = _capi.load()
    if pool not in _EXAM_POOL:
        raise ValueError("pool must be None, 'max' or 'ave'")
    R = R_img.contiguous()
    if R.dtype not in (torch.float32, torch.float64) or R.dim() != 4:
        raise ValueError("expected an (n, H, W, C) float32 or float64 tensor")
    n, Hh, Ww, Cc = R.shape
    k = int(k) if pool is not None else 1
    if pool is not None and (k < 1 or Hh % k or Ww % k):
        raise ValueError("the pool block k must divide H and W")
    maps = None
    if want_maps:
        maps = torch.empty((n, Hh // k, Ww // k), dtype=R.dtype if pool is None else torch.float64, device=R.device)
    means = torch.empty((n,), dtype=torch.float64, device=R.device)
    _capi.check(lib.lrp_exam_maps(C.c_void_p(R.data_ptr()), int(R.dtype == torch.float64), n, Hh, Ww, Cc, _EXAM_POOL[pool], k,
                                  int(bool(absval)), C.c_void_p(maps.data_ptr()) if maps is not None else None,
                                  C.c_void_p(means.data_ptr()), _cur_stream(R.device)))
    return maps, means


# ---- perturbation analysis (innvestigate/tools/perturbate.py, PT:; csrc/perturb_kernels.h, lrp_perturb_*)
PERTURB_MAX_REGIONS = 4096
_PERTURB_FN = {"mean": 0, "max": 1}
_PERTURB_MODE = {"zeros": 0, "mean": 1, "invert": 2, "noise": 3}


def perturb_geometry(H, W, region_shape):
    """The region grid of PT:105-116 / PT:170 (host arithmetic): (Hr, Wr, rows padded before, columns padded before).
    ValueError when the region divides exactly one axis (the reference's assert, PT:107); NotImplementedError for a region
    side below 1 or more than PERTURB_MAX_REGIONS regions."""
    rh, rw = int(region_shape[0]), int(region_shape[1])
    if rh < 1 or rw < 1:
        raise NotImplementedError("the region shape must be at least 1 x 1")
    dh, dw = H % rh == 0, W % rw == 0
    if dh != dw:
        raise ValueError("region (%d, %d) divides one axis of (%d, %d) and not the other: the reference pads the divisible "
                         "axis by a whole region and fails its assert (perturbate.py:107)" % (rh, rw, H, W))
    ph, pw = (0 if dh else rh - H % rh), (0 if dw else rw - W % rw)
    Hr, Wr = (H + ph) // rh, (W + pw) // rw
    if Hr * Wr > PERTURB_MAX_REGIONS:
        raise NotImplementedError("%d regions: at most %d are ranked" % (Hr * Wr, PERTURB_MAX_REGIONS))
    return Hr, Wr, ph // 2, pw // 2


def perturb_ranks(R_img, region_shape, reduce="mean", aggregate="mean", want_scores=False, negate=False):
    """Region ranks of PT:79-84 on the device: R_img (n, H, W, C) float32 or float64 tensor -> ranks (n, nreg) int32, 0 = the
    most relevant region, exact ties to the lower region index, NaN last; with want_scores also the (n, nreg) float64 region
    scores (channel `reduce`, region `aggregate`, each 'mean' or 'max'; negated if `negate`: least relevant first)."""
    lib = _capi.load()
    if reduce not in _PERTURB_FN or aggregate not in _PERTURB_FN:
        raise ValueError("reduce and aggregate must be 'mean' or 'max'")
    R = R_img.contiguous()
    if R.dtype not in (torch.float32, torch.float64) or R.dim() != 4:
        raise ValueError("expected an (n, H, W, C) float32 or float64 tensor")
    n, Hh, Ww, Cc = R.shape
    Hr, Wr, _, _ = perturb_geometry(Hh, Ww, region_shape)
    ranks = torch.empty((n, Hr * Wr), dtype=torch.int32, device=R.device)
    scores = torch.empty((n, Hr * Wr), dtype=torch.float64, device=R.device) if want_scores else None
    _capi.check(lib.lrp_perturb_ranks(C.c_void_p(R.data_ptr()), int(R.dtype == torch.float64), n, Hh, Ww, Cc,
                                      int(region_shape[0]), int(region_shape[1]), _PERTURB_FN[reduce], _PERTURB_FN[aggregate],
                                      int(bool(negate)), C.c_void_p(ranks.data_ptr()),
                                      C.c_void_p(scores.data_ptr()) if scores is not None else None, _cur_stream(R.device)))
    return (ranks, scores) if want_scores else ranks


def perturb_apply(x, img_idx, ranks, k, region_shape, mode="zeros", noise=None, all_channels=False, value_range=None):
    """PT:130-148 on the device: x (B, H, W, C) float32 tensor, img_idx (n) image index per unit, ranks (n, nreg) int32 tensor,
    k (n) or a scalar: the regions of rank <= k - 1 are replaced -> (n, H, W, C) float32 tensor.  mode 'zeros' | 'mean' |
    'invert' | 'noise' (copies `noise` (n, H, W, C) inside the perturbed regions); channel 0 only unless all_channels;
    value_range (lo, hi): a unit with k >= 1 is clipped, perturbed and clipped again.  A unit whose image index is outside
    [0, B) comes out as NaN."""
    lib = _capi.load()
    if mode not in _PERTURB_MODE:
        raise ValueError("mode must be 'zeros', 'mean', 'invert' or 'noise'")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("expected a (B, H, W, C) float32 tensor")
    x = x.contiguous()
    B, Hh, Ww, Cc = x.shape
    Hr, Wr, _, _ = perturb_geometry(Hh, Ww, region_shape)
    dev = x.device
    if ranks.dtype != torch.int32 or ranks.dim() != 2 or ranks.shape[1] != Hr * Wr or ranks.device != dev:
        raise ValueError("ranks must be an (n, %d) int32 tensor on the device of x" % (Hr * Wr))
    ranks = ranks.contiguous()
    n = ranks.shape[0]
    idx = img_idx if torch.is_tensor(img_idx) else torch.as_tensor(np.asarray(img_idx, dtype=np.int32).reshape(-1))
    idx = idx.to(device=dev, dtype=torch.int32).contiguous()
    kk = k if torch.is_tensor(k) else torch.as_tensor(np.broadcast_to(np.asarray(k, dtype=np.float64), (n,)).copy())
    kk = kk.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(idx.shape) != (n,) or tuple(kk.shape) != (n,):
        raise ValueError("img_idx and k must hold one entry per row of ranks")
    if (mode == "noise") != (noise is not None):
        raise ValueError("`noise` goes with mode 'noise' and with no other")
    if noise is not None:
        if noise.dtype != torch.float32 or tuple(noise.shape) != (n, Hh, Ww, Cc) or noise.device != dev:
            raise ValueError("noise must be an (n, H, W, C) float32 tensor on the device of x")
        noise = noise.contiguous()
    lo, hi = (0.0, 0.0) if value_range is None else (float(value_range[0]), float(value_range[1]))
    out = torch.empty((n, Hh, Ww, Cc), dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _capi.check(lib.lrp_perturb_apply(p(x), p(idx), p(ranks), p(kk), p(noise), p(out), n, B, Hh, Ww, Cc, int(region_shape[0]),
                                      int(region_shape[1]), _PERTURB_MODE[mode], int(bool(all_channels)),
                                      int(value_range is not None), C.c_float(lo), C.c_float(hi), _cur_stream(dev)))
    return out


def perturb_word_scores(engine, slot, t, col):
    """The score of n words on the cached forward of `engine` (an LRPEngine after decoder_forward), read in place: slot, t,
    col (n) ints (lists or device tensors): image slot, position t >= 1, model column (token id - 1) -> (logit, logp), (n,)
    float64 device tensors: l[col] and log_softmax(l)[col] of row t - 1 of caption_preds.  A unit outside the cached logits
    comes out as NaN."""
    def dev(a):
        a = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, dtype=np.int32).reshape(-1))
        return a.to(device=engine.device, dtype=torch.int32).contiguous()
    s, tt, kk = dev(slot), dev(t), dev(col)
    n = s.shape[0]
    if n < 1 or tuple(tt.shape) != (n,) or tuple(kk.shape) != (n,):
        raise ValueError("slot, t and col must hold the same number (>= 1) of entries")
    logit = torch.empty((n,), dtype=torch.float64, device=engine.device)
    logp = torch.empty((n,), dtype=torch.float64, device=engine.device)
    p = lambda x: C.c_void_p(x.data_ptr())
    _capi.check(engine._lib.lrp_perturb_word_scores(engine._h, p(s), p(tt), p(kk), n, p(logit), p(logp), engine._stream()))
    return logit, logp


# ---- occlusion and RISE word saliency (csrc/saliency_kernels.h, lrp_op_occlude / _occlusion_map / _rise_*)
OCC_MAX_WINDOWS = 65536
RISE_MAX_S = 63


def _pair(v, what):
    try:
        a, b = (v, v) if np.isscalar(v) else v
        a, b = int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError("%s must be an int or a pair of ints" % what)
    return a, b


def occlusion_geometry(H, W, window, stride=None):
    """(Hn, Wn): windows per column / row (host arithmetic of include/lrp_hip.h).  stride None: the window.  ValueError unless
    1 <= stride <= window <= image on both axes; NotImplementedError for more than OCC_MAX_WINDOWS windows."""
    ph, pw = _pair(window, "window")
    sh, sw = (ph, pw) if stride is None else _pair(stride, "stride")
    if not (1 <= sh <= ph <= H and 1 <= sw <= pw <= W):
        raise ValueError("occlusion needs 1 <= stride <= window <= image on both axes: window (%d, %d), stride (%d, %d), image "
                         "(%d, %d)" % (ph, pw, sh, sw, H, W))
    Hn, Wn = -(-(H - ph) // sh) + 1, -(-(W - pw) // sw) + 1
    if Hn * Wn > OCC_MAX_WINDOWS:
        raise NotImplementedError("%d windows: at most %d are scored" % (Hn * Wn, OCC_MAX_WINDOWS))
    return Hn, Wn


def rise_cell(H, W, s):
    """(ch, cw) = (ceil(H / s), ceil(W / s)): the smallest cell whose (s + 1)^2 grid covers the image at every shift."""
    s = int(s)
    if not 1 <= s <= RISE_MAX_S:
        raise NotImplementedError("RISE grid s=%d outside [1,%d]" % (s, RISE_MAX_S))
    return -(-H // s), -(-W // s)


def _sal_images(x):
    if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4 or not x.is_cuda:
        raise ValueError("expected a (B, H, W, C) float32 device tensor")
    return x.contiguous()


def _sal_ints(a, dev, n=None, dtype=torch.int32, shape=None):
    if not torch.is_tensor(a):
        a = torch.as_tensor(np.asarray(a, dtype=np.int64))
    a = a.to(device=dev, dtype=dtype).contiguous()
    want = shape if shape is not None else ((n,) if n is not None else (a.numel(),))
    if tuple(a.shape) != tuple(want):
        raise ValueError("expected %s entries, got %s" % (tuple(want), tuple(a.shape)))
    return a


def _sal_fill(fill, Cc, dev):
    f = np.asarray(fill, dtype=np.float32).reshape(-1)
    if f.size not in (1, Cc):
        raise ValueError("fill must be a scalar or one value per channel (%d)" % Cc)
    return torch.as_tensor(np.broadcast_to(f, (Cc,)).copy()).to(dev)


def op_occlude(x, img_idx, k, window, stride=None, fill=0.0):
    """x (B, H, W, C) float32 device tensor -> (n, H, W, C): row r is image img_idx[r] with occlusion window k[r] set to `fill`
    (a scalar, one value per channel, or a (C,) device tensor), every channel; k = -1 copies the image.  An image index outside
    [0, B) or a k outside [-1, Hn * Wn) gives a NaN row."""
    x = _sal_images(x)
    B, Hh, Ww, Cc = x.shape
    ph, pw = _pair(window, "window")
    sh, sw = (ph, pw) if stride is None else _pair(stride, "stride")
    dev = x.device
    idx = _sal_ints(img_idx, dev)
    n = idx.shape[0]
    kk = _sal_ints(k, dev, n)
    f = fill.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(fill) else _sal_fill(fill, Cc, dev)
    if tuple(f.shape) != (Cc,):
        raise ValueError("fill must hold one value per channel")
    out = torch.empty((n, Hh, Ww, Cc), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().lrp_op_occlude(_p(x), _p(idx), _p(kk), _p(f), _p(out), n, B, Hh, Ww, Cc, ph, pw, sh, sw,
                                            _cur_stream(dev)))
    return out


def op_occlusion_map(scores, H, W, window, stride=None):
    """scores (n_img, 1 + Hn * Wn, T) float64 device tensor, row 0 the unoccluded score -> (n_img, T, H, W) float32: per pixel
    the mean over the covering windows of s_0 - s_window, summed in float64 in ascending window order."""
    ph, pw = _pair(window, "window")
    sh, sw = (ph, pw) if stride is None else _pair(stride, "stride")
    Hn, Wn = occlusion_geometry(H, W, (ph, pw), (sh, sw))
    if not torch.is_tensor(scores) or scores.dtype != torch.float64 or scores.dim() != 3 or scores.shape[1] != 1 + Hn * Wn:
        raise ValueError("scores must be an (n_img, %d, T) float64 device tensor" % (1 + Hn * Wn))
    scores = scores.contiguous()
    n_img, _, T = scores.shape
    out = torch.empty((n_img, T, H, W), dtype=torch.float32, device=scores.device)
    _capi.check(_capi.load().lrp_op_occlusion_map(_p(scores), _p(out), n_img, T, H, W, ph, pw, sh, sw, _cur_stream(scores.device)))
    return out


def op_rise_grids(keys, k, s, p, seed, H, W, cell=None, device=None):
    """Masks (key, k) -> (grid (n, (s + 1)^2) uint8, shift (n, 2) int32) device tensors: Philox4x32-10 draws that depend on
    (seed, key, k) alone (include/lrp_hip.h).  keys: the caller's identity of each row's image (uint32); cell: (ch, cw), default
    rise_cell(H, W, s)."""
    ch, cw = rise_cell(H, W, s) if cell is None else _pair(cell, "cell")
    dev = device if device is not None else (k.device if torch.is_tensor(k) else torch.device("cuda", torch.cuda.current_device()))
    kk = _sal_ints(k, dev)
    n = kk.shape[0]
    ky = _sal_ints(keys, dev, n, dtype=torch.int64) & 0xFFFFFFFF            # the uint32's bits in an int32 tensor
    ky = torch.where(ky >= 2 ** 31, ky - 2 ** 32, ky).to(torch.int32).contiguous()
    grid = torch.empty((n, (int(s) + 1) ** 2), dtype=torch.uint8, device=dev)
    shift = torch.empty((n, 2), dtype=torch.int32, device=dev)
    _capi.check(_capi.load().lrp_op_rise_grids(_p(ky), _p(kk), n, int(s), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, H, W, ch, cw,
                                               _p(grid), _p(shift), _cur_stream(dev)))
    return grid, shift


def op_rise_apply(x, img_idx, grid, shift, s, fill=0.0, cell=None):
    """x (B, H, W, C) float32 device tensor -> (n, H, W, C): fill + m (x - fill), row r from image img_idx[r] under the mask of
    grid[r] / shift[r] (op_rise_grids): the (s + 1)^2 grid upsampled bilinearly by `cell` pixels per cell, cropped at the shift."""
    x = _sal_images(x)
    B, Hh, Ww, Cc = x.shape
    ch, cw = rise_cell(Hh, Ww, s) if cell is None else _pair(cell, "cell")
    dev = x.device
    idx = _sal_ints(img_idx, dev)
    n = idx.shape[0]
    if grid.dtype != torch.uint8 or tuple(grid.shape) != (n, (int(s) + 1) ** 2) or grid.device != dev:
        raise ValueError("grid must be an (n, (s + 1)^2) uint8 tensor on the device of x")
    sh = _sal_ints(shift, dev, shape=(n, 2))
    f = fill.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(fill) else _sal_fill(fill, Cc, dev)
    if tuple(f.shape) != (Cc,):
        raise ValueError("fill must hold one value per channel")
    out = torch.empty((n, Hh, Ww, Cc), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().lrp_op_rise_apply(_p(x), _p(idx), _p(grid.contiguous()), _p(sh), _p(f), _p(out), n, B, Hh, Ww, Cc,
                                               int(s), ch, cw, _cur_stream(dev)))
    return out


def op_rise_map(scores, grid, shift, H, W, s, p, cell=None):
    """scores (n_img, K, T) float64, grid (n_img, K, (s + 1)^2) uint8, shift (n_img, K, 2) int32 device tensors ->
    (n_img, T, H, W) float32: sum_k s_k[t] m_k(y, x) / (K p), the masks recomputed from the grids, summed in float64 in ascending
    k whatever else shares the launch."""
    ch, cw = rise_cell(H, W, s) if cell is None else _pair(cell, "cell")
    if not torch.is_tensor(scores) or scores.dtype != torch.float64 or scores.dim() != 3:
        raise ValueError("scores must be an (n_img, K, T) float64 device tensor")
    scores = scores.contiguous()
    n_img, K, T = scores.shape
    dev = scores.device
    if grid.dtype != torch.uint8 or tuple(grid.shape) != (n_img, K, (int(s) + 1) ** 2) or grid.device != dev:
        raise ValueError("grid must be an (n_img, K, (s + 1)^2) uint8 tensor on the device of the scores")
    sh = _sal_ints(shift, dev, shape=(n_img, K, 2))
    out = torch.empty((n_img, T, H, W), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().lrp_op_rise_map(_p(scores), _p(grid.contiguous()), _p(sh), _p(out), n_img, K, T, H, W, int(s), float(p),
                                             ch, cw, _cur_stream(dev)))
    return out


# ---- the CAM family as word saliencies (csrc/cam_kernels.h, lrp_op_cam / _cam_weighted / _scorecam_apply / _feature_ablate)
CAM_MODES = {"gradcam": 0, "gradcam++": 1, "xgradcam": 2, "layercam": 3, "hirescam": 4}
CAM_WEIGHTS = {"softmax": 0, "linear": 1, "ablation": 2}
CAM_MAX_G, CAM_MAX_S, CAM_MAX_D = 16, 448, 4096


def cam_geometry(L, H, W):
    """(g, upscale) of an (H, W) image over L = g * g feature positions.  ValueError unless the image is square and its side a
    multiple of sqrt(L); NotImplementedError beyond g = 16 or a side of 448."""
    g = int(round(np.sqrt(L)))
    if g < 1 or g * g != L or H != W or H < g or H % g != 0:
        raise ValueError("the CAM family needs a square image whose side is a multiple of sqrt(L): image (%d, %d), L=%d" % (H, W, L))
    if g > CAM_MAX_G or H > CAM_MAX_S:
        raise NotImplementedError("the CAM kernels take g <= %d and an image side <= %d" % (CAM_MAX_G, CAM_MAX_S))
    return g, H // g


def _cam_channels(D):
    if D < 8 or D % 8 != 0 or D > CAM_MAX_D:
        raise ValueError("D must be a multiple of 8 in [8, %d] (D=%d)" % (CAM_MAX_D, D))


def _cam_features(feat, g):
    if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 3 or feat.shape[1] != g * g or not feat.is_cuda:
        raise ValueError("expected a (B, g * g, D) float32 device tensor of features")
    return feat.contiguous()


def op_cam(feat, img_idx, grads, g, upscale, method="gradcam", gb=None, sigma=20.0):
    """The gradient forms of the CAM family for n (image, word) units in fp64 on the device: feat (B, L, D) float32 device
    tensor, img_idx n image indices, grads (n, L, D) float32, L = g * g, method one of CAM_MODES -> cam (n, S, S) float64,
    S = g * upscale.  With gb (n, S, S, C) float32 -> (gb * cam (n, S, S, C) float64, cam).  method='gradcam' equals op_gradcam
    bit for bit.  A unit whose image index is outside [0, B) comes out as NaN."""
    if method not in CAM_MODES:
        raise ValueError("unknown CAM method %r: one of %s" % (method, sorted(CAM_MODES)))
    g, upscale = int(g), int(upscale)
    if not (1 <= g <= CAM_MAX_G and upscale >= 1 and g * upscale <= CAM_MAX_S):
        raise ValueError("need 1 <= g <= %d and 1 <= g * upscale <= %d" % (CAM_MAX_G, CAM_MAX_S))
    if not torch.is_tensor(feat) or not torch.is_tensor(grads) or feat.dim() != 3 or grads.dim() != 3:
        raise ValueError("expected feat (B, g * g, D) and grads (n, g * g, D) float32 tensors")
    _cam_channels(int(feat.shape[2]))
    f = _cam_features(feat, g)
    d = grads.contiguous()
    if d.dtype != torch.float32 or tuple(d.shape[1:]) != tuple(f.shape[1:]) or d.device != f.device:
        raise ValueError("expected feat (B, g * g, D) and grads (n, g * g, D) float32 tensors on one device")
    n, B, D, S = d.shape[0], f.shape[0], f.shape[2], g * upscale
    idx = _sal_ints(img_idx, f.device, n)
    out = None
    if gb is not None:
        gb = gb.contiguous()
        if gb.dtype != torch.float32 or gb.dim() != 4 or tuple(gb.shape[:3]) != (n, S, S) or not 1 <= gb.shape[3] <= 64:
            raise ValueError("gb must be an (n, S, S, C) float32 tensor, C <= 64")
        out = torch.empty(gb.shape, dtype=torch.float64, device=f.device)
    M = _expand_matrix_dev(f.device, g, upscale, sigma)
    cam = torch.empty((n, S, S), dtype=torch.float64, device=f.device)
    _capi.check(_capi.load().lrp_op_cam(_p(f), _p(idx), _p(d), _p(M), _p(gb), _p(cam), _p(out), n, B, g, upscale, D,
                                        gb.shape[3] if gb is not None else 0, CAM_MODES[method], _cur_stream(f.device)))
    return cam if gb is None else (out, cam)


def op_cam_weighted(scores, feat, img_idx, g, upscale, weights="softmax", want_cam=False, sigma=20.0):
    """The fold of Score-CAM and Ablation-CAM: scores (n_img, R, T) float64 device tensor (row 0 the unmasked image, row 1 + k
    channel k, with 'linear' row 1 + D the fill image), feat (B, L, D) float32, img_idx n_img rows of feat, weights one of
    CAM_WEIGHTS -> (n_img, T, S, S) float32 maps (want_cam: (maps, the float64 cams they were rounded from))."""
    if weights not in CAM_WEIGHTS:
        raise ValueError("unknown weighting %r: one of %s" % (weights, sorted(CAM_WEIGHTS)))
    g, upscale = int(g), int(upscale)
    if not (1 <= g <= CAM_MAX_G and upscale >= 1 and g * upscale <= CAM_MAX_S):
        raise ValueError("need 1 <= g <= %d and 1 <= g * upscale <= %d" % (CAM_MAX_G, CAM_MAX_S))
    if not torch.is_tensor(feat) or feat.dim() != 3:
        raise ValueError("expected a (B, g * g, D) float32 device tensor of features")
    D = int(feat.shape[2])
    _cam_channels(D)
    f = _cam_features(feat, g)
    R = 1 + D + (weights == "linear")
    if not torch.is_tensor(scores) or scores.dtype != torch.float64 or scores.dim() != 3 or scores.shape[1] != R \
            or scores.device != f.device or scores.shape[2] < 1:
        raise ValueError("scores must be an (n_img, %d, T) float64 tensor on the device of the features" % R)
    scores = scores.contiguous()
    n_img, _, T = scores.shape
    idx = _sal_ints(img_idx, f.device, n_img)
    S = g * upscale
    M = _expand_matrix_dev(f.device, g, upscale, sigma)
    maps = torch.empty((n_img, T, S, S), dtype=torch.float32, device=f.device)
    cam = torch.empty((n_img, T, S, S), dtype=torch.float64, device=f.device) if want_cam else None
    _capi.check(_capi.load().lrp_op_cam_weighted(_p(scores), _p(f), _p(idx), _p(M), _p(cam), _p(maps), n_img, R, T, f.shape[0], g,
                                                 upscale, D, CAM_WEIGHTS[weights], _cur_stream(f.device)))
    return (maps, cam) if want_cam else maps


def op_scorecam_apply(x, feat, img_idx, k, g, upscale, fill=0.0):
    """x (B, H, W, C) float32 device tensor, H = W = g * upscale, feat (B, g * g, D) -> (n, H, W, C): row r is fill + m (x - fill)
    with m the min-max normalised, bilinearly upsampled map of channel k[r] of image img_idx[r]; k = -1 copies the image, k = D
    gives the fill image; an image index outside [0, B) or a k outside [-1, D] gives a NaN row."""
    x = _sal_images(x)
    B, Hh, Ww, Cc = x.shape
    g, upscale = int(g), int(upscale)
    if not (1 <= g <= CAM_MAX_G and upscale >= 1) or Hh != Ww or Hh != g * upscale:
        raise ValueError("need a square image of side g * upscale, 1 <= g <= %d: image (%d, %d), g=%d, upscale=%d"
                         % (CAM_MAX_G, Hh, Ww, g, upscale))
    f = _cam_features(feat, g)
    dev = x.device
    if f.device != dev or f.shape[0] != B:
        raise ValueError("feat must hold the features of the B images, on their device")
    idx = _sal_ints(img_idx, dev)
    n = idx.shape[0]
    if not 1 <= n <= 65535:
        raise ValueError("between 1 and 65535 rows per call")
    kk = _sal_ints(k, dev, n)
    fl = fill.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(fill) else _sal_fill(fill, Cc, dev)
    if tuple(fl.shape) != (Cc,):
        raise ValueError("fill must hold one value per channel")
    out = torch.empty((n, Hh, Ww, Cc), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().lrp_op_scorecam_apply(_p(x), _p(f), _p(idx), _p(kk), _p(fl), _p(out), n, B, g, upscale, Cc,
                                                   int(f.shape[2]), _cur_stream(dev)))
    return out


def op_feature_ablate(feat, img_idx, k):
    """feat (B, L, D) float32 device tensor -> (n, L, D): row r is feat[img_idx[r]] with channel k[r] set to 0; k = -1 copies;
    an image index outside [0, B) or a k outside [-1, D) gives a NaN row."""
    if not torch.is_tensor(feat) or feat.dtype != torch.float32 or feat.dim() != 3 or not feat.is_cuda:
        raise ValueError("expected a (B, L, D) float32 device tensor of features")
    f = feat.contiguous()
    B, L, D = f.shape
    idx = _sal_ints(img_idx, f.device)
    n = idx.shape[0]
    if n < 1:
        raise ValueError("at least one row")
    kk = _sal_ints(k, f.device, n)
    out = torch.empty((n, L, D), dtype=torch.float32, device=f.device)
    _capi.check(_capi.load().lrp_op_feature_ablate(_p(f), _p(idx), _p(kk), _p(out), n, B, L, D, _cur_stream(f.device)))
    return out


# ---- LIME and KernelSHAP word saliency (csrc/segment_kernels.h, lrp_op_segment_*)
SEG_MAX_D = 128
SEG_MODES = {"bernoulli": 0, "shapley": 1}


def _seg_count(d):
    d = int(d)
    if not 2 <= d <= SEG_MAX_D:
        raise NotImplementedError("segment count d=%d outside [2,%d]" % (d, SEG_MAX_D))
    return d


def shapley_size_thresholds(d):
    """(d - 2,) uint32: thr[i] = min(2^32 - 1, floor(C(i + 1) 2^32)) in float64, C the cumulative of the Shapley kernel's size
    distribution p(m) ~ (d - 1) / (m (d - m)), m = 1 .. d - 1.  A uniform 32-bit u has size 1 + #{i : u >= thr[i]}: the integers
    lrp_op_segment_draws compares against."""
    d = _seg_count(d)
    m = np.arange(1, d, dtype=np.float64)
    pm = (d - 1.0) / (m * (d - m))
    cum = np.cumsum(pm / pm.sum())[:d - 2]
    return np.minimum(2.0 ** 32 - 1.0, np.floor(cum * 2.0 ** 32)).astype(np.uint32)


def _seg_bits(bits, dev, shape):
    if not torch.is_tensor(bits):
        bits = torch.as_tensor(np.ascontiguousarray(np.asarray(bits).astype(np.uint32)).view(np.int32))
    if bits.dtype != torch.int32 or tuple(bits.shape) != tuple(shape):
        raise ValueError("bits must be a %s int32 tensor (the uint32 words' bits)" % (tuple(shape),))
    return bits.to(dev).contiguous()


def _seg_labels(label, dev, shape):
    if not torch.is_tensor(label):
        label = torch.as_tensor(np.asarray(label, dtype=np.int64))
    if tuple(label.shape) != tuple(shape):
        raise ValueError("labels must be %s ints" % (tuple(shape),))
    return label.to(device=dev, dtype=torch.int32).contiguous()


def op_segment_draws(keys, k, d, mode, p=0.5, seed=0, device=None):
    """Rows (key, k) -> (n, 4) int32 device tensor holding the uint32 words of each row's subset of d segments: bit j of word
    j / 32 is segment j.  mode 'bernoulli' (each segment on with probability p) or 'shapley' (size from the Shapley kernel's
    distribution, then a uniform subset of that size; an odd k the complement of k - 1).  Philox4x32-10 draws that depend on
    (seed, key, k, d, p) alone (include/lrp_hip.h)."""
    d = _seg_count(d)
    if mode not in SEG_MODES:
        raise ValueError("mode must be 'bernoulli' or 'shapley'")
    dev = device if device is not None else (k.device if torch.is_tensor(k) else torch.device("cuda", torch.cuda.current_device()))
    kk = _sal_ints(k, dev)
    n = kk.shape[0]
    ky = _sal_ints(keys, dev, n, dtype=torch.int64) & 0xFFFFFFFF            # the uint32's bits in an int32 tensor
    ky = torch.where(ky >= 2 ** 31, ky - 2 ** 32, ky).to(torch.int32).contiguous()
    thr = None
    if mode == "shapley" and d > 2:
        thr = torch.as_tensor(shapley_size_thresholds(d).view(np.int32)).to(dev)
    bits = torch.empty((n, 4), dtype=torch.int32, device=dev)
    _capi.check(_capi.load().lrp_op_segment_draws(_p(ky), _p(kk), n, d, SEG_MODES[mode], float(p), None if thr is None else _p(thr),
                                                  int(seed) & 0xFFFFFFFFFFFFFFFF, _p(bits), _cur_stream(dev)))
    return bits


def op_segment_apply(x, img_idx, bits, label, d, fill=0.0):
    """x (B, H, W, C) float32 device tensor, label (B, H, W) ints in [0, d) -> (n, H, W, C): row r is image img_idx[r] with the
    pixels of every segment that is off in bits[r] set to `fill`; values are selected, never computed.  An image index outside
    [0, B) gives a NaN row, a label outside [0, d) a NaN pixel."""
    x = _sal_images(x)
    B, Hh, Ww, Cc = x.shape
    d = _seg_count(d)
    dev = x.device
    idx = _sal_ints(img_idx, dev)
    n = idx.shape[0]
    bits = _seg_bits(bits, dev, (n, 4))
    label = _seg_labels(label, dev, (B, Hh, Ww))
    f = fill.to(device=dev, dtype=torch.float32).contiguous() if torch.is_tensor(fill) else _sal_fill(fill, Cc, dev)
    if tuple(f.shape) != (Cc,):
        raise ValueError("fill must hold one value per channel")
    out = torch.empty((n, Hh, Ww, Cc), dtype=torch.float32, device=dev)
    _capi.check(_capi.load().lrp_op_segment_apply(_p(x), _p(idx), _p(bits), _p(label), _p(f), _p(out), n, B, Hh, Ww, Cc, d,
                                                  _cur_stream(dev)))
    return out


def op_segment_fit(bits, wtab, y, d, ridge=0.0, delta=None):
    """bits (n_img, K, 4) int32, wtab (d + 1,) float64 (the row weight by subset size), y (n_img, K, T) float64 device tensors ->
    (phi (n_img, T, d), intercept (n_img, T), status (n_img,) int32).  delta None: weighted ridge regression of y on the
    subsets with a free intercept (LIME); delta (n_img, T): the Shapley form, sum(phi) = delta by elimination, intercept 0.
    status 1: the normal equations are singular (phi NaN)."""
    d = _seg_count(d)
    if not torch.is_tensor(y) or y.dtype != torch.float64 or y.dim() != 3 or not y.is_cuda:
        raise ValueError("y must be an (n_img, K, T) float64 device tensor")
    y = y.contiguous()
    n_img, K, T = y.shape
    dev = y.device
    bits = _seg_bits(bits, dev, (n_img, K, 4))
    wt = torch.as_tensor(np.ascontiguousarray(wtab, dtype=np.float64)) if not torch.is_tensor(wtab) else wtab
    wt = wt.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(wt.shape) != (d + 1,):
        raise ValueError("wtab must hold d + 1 weights")
    if delta is not None:
        if not torch.is_tensor(delta) or delta.dtype != torch.float64 or tuple(delta.shape) != (n_img, T) or delta.device != dev:
            raise ValueError("delta must be an (n_img, T) float64 tensor on the device of y")
        delta = delta.contiguous()
    phi = torch.empty((n_img, T, d), dtype=torch.float64, device=dev)
    icpt = torch.empty((n_img, T), dtype=torch.float64, device=dev)
    status = torch.empty((n_img,), dtype=torch.int32, device=dev)
    _capi.check(_capi.load().lrp_op_segment_fit(_p(bits), _p(wt), _p(y), None if delta is None else _p(delta), float(ridge), _p(phi),
                                                _p(icpt), _p(status), n_img, K, T, d, _cur_stream(dev)))
    return phi, icpt, status


def op_segment_map(phi, label, d):
    """phi (n_img, T, d) float64, label (n_img, H, W) ints -> (n_img, T, H, W) float32: phi[t][label], rounded once; NaN for a
    label outside [0, d)."""
    d = _seg_count(d)
    if not torch.is_tensor(phi) or phi.dtype != torch.float64 or phi.dim() != 3 or phi.shape[2] != d or not phi.is_cuda:
        raise ValueError("phi must be an (n_img, T, d) float64 device tensor")
    phi = phi.contiguous()
    n_img, T, _ = phi.shape
    if not hasattr(label, "shape") or len(label.shape) != 3 or label.shape[0] != n_img:
        raise ValueError("labels must be (n_img, H, W) ints")
    H, W = int(label.shape[1]), int(label.shape[2])
    label = _seg_labels(label, phi.device, (n_img, H, W))
    out = torch.empty((n_img, T, H, W), dtype=torch.float32, device=phi.device)
    _capi.check(_capi.load().lrp_op_segment_map(_p(phi), _p(label), _p(out), n_img, T, H, W, d, _cur_stream(phi.device)))
    return out
