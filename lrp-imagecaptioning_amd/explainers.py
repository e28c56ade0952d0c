"""Engine classes with the reference's explainer protocol (models/explainers.py, cited E:).

    ExplainImgCaptioningAttentionModel      E:22-256   (base: CNN analyzer, _explain_CNN, _explain_sentence)
    ExplainImgCaptioningAdaptiveAttention   E:260-666
    ExplainImgCaptioningGridTDModel         E:995-1321

Same method names, argument meaning, return shapes/dtypes and error behaviour, so
that `explain_image.Explainer`-style harnesses (explain_image.py:4-183) can drive
them unchanged.  What differs is construction: there is no Keras model to pull
weights from, so `model` is a `CaptionModelSpec` (geometry + a dict of arrays in
the Keras layouts) and `weight_path` may name an `.npz` bundle of those arrays
(hdf5 is not available).  All arithmetic runs in liblrp_hip.so through LRPEngine;
these classes hold no math of their own.
"""
import numpy as np
import torch

from .engine import LRPEngine
from .synthetic import VGG16_CFG

EPS = 0.01      # E:18  (CNN analyzer epsilon; only Dense layers use it, none in the truncated VGG16)
ALPHA = 1       # E:19
BETA = 0        # E:20


class CaptionPreprocessorStub(object):
    """The two attributes of models/preprocessors.py:CaptionPreprocessorAttention the hot path reads."""

    def __init__(self, sos=2, eos=1, word_of=None):
        self.SOS_TOKEN_LABEL_ENCODED = sos
        self.EOS_TOKEN_LABEL_ENCODED = eos
        self._word_of = word_of or {}

    def decode_captions_from_list1d(self, ids):
        return " ".join(self._word_of.get(int(i), "<%d>" % int(i)) for i in ids if int(i) != self.EOS_TOKEN_LABEL_ENCODED)


class DatasetProviderStub(object):
    def __init__(self, caption_preprocessor=None, image_preprocessor=None):
        self.caption_preprocessor = caption_preprocessor or CaptionPreprocessorStub()
        self.image_preprocessor = image_preprocessor


class CaptionModelSpec(object):
    """What the reference reads off `model` (E:26-39): encoder kind, dims, and the weights."""

    def __init__(self, weights, img_encoder="vgg16", hidden_dim=512, embedding_dim=512, L=196, D=512,
                 vocab_size=None, cnn_cfg=None, img_hw=(224, 224), resnet=None, cnn_rule=(1, 0)):
        """cnn_rule: the (alpha, beta) of the encoder's conv rule (LRPEngine.set_cnn_rule), or 'alpha1beta0' (the default:
        LRPSequentialPresetA, E:32) / 'alpha2beta1' (LRPSequentialPresetB's conv rule), or a preset name of analyzer.PRESETS
        ('presetB', and — VGG-style encoders — 'presetAflat', 'presetBflat', 'zplus', ...) or a list with one rule per conv, input
        layer first, or a dict {"rule": ..., "input_layer_rule": ...} with the keywords of analyzer.LRP(...) — either encoder: a
        VGG-style one makes analyzer.rule_table of it, a ResNet one the rule pair of LRPEngine.set_resnet_rules (self.cnn_rules is
        then (stem record, record of the other convs)).  The preset names and lists on a ResNet encoder take what amounts to ONE
        alpha-beta rule with bias on every conv (NotImplementedError otherwise)
        (analyzer.normalize_rule; LRPEngine.set_cnn_rules: self.cnn_rules holds the table, self.cnn_rule is then None); every explainer built on the spec
        whose CNN half is the LRP walk applies it to its engine; the gradient-baseline classes do not (their walks ignore the
        rule, and setting it would cost them its encode pass and buffers for nothing).
        img_encoder 'vgg16' (config.py:36-40: block5_conv3, 196 x 512), 'vgg19' (config.py:37: block5_conv4) or
        'resnet101' (config.py:41-45: conv5_block3_out, 49 x 2048; `resnet` = dict(stem, stacks), default ResNet-101).
        cnn_cfg: the conv list of a VGG-style encoder (default: the full-size one of `img_encoder`)."""
        if img_encoder not in ("vgg16", "vgg19", "resnet101"):
            raise NotImplementedError("the img_encode is not valid, [vgg16, vgg19, resnet101]")     # explain_image.py:25-26
        if cnn_cfg is None:
            from .synthetic import VGG19_CFG
            cnn_cfg = VGG19_CFG if img_encoder == "vgg19" else VGG16_CFG
        if img_encoder == "resnet101" and resnet is None:
            from .synthetic import RESNET101_STACKS
            resnet = {"stem": 64, "stacks": RESNET101_STACKS}
        self.resnet = resnet if img_encoder == "resnet101" else None
        self.weights = dict(weights)
        self.img_encoder = img_encoder
        self._hidden_dim, self._embedding_dim = hidden_dim, embedding_dim
        self.L, self.D = L, D
        self.vocab_size = vocab_size if vocab_size is not None else int(self.weights["output_W"].shape[1])
        self.cnn_cfg = list(cnn_cfg)
        self.img_hw = tuple(img_hw)
        from .analyzer import PRESETS, infer_alpha_beta, rule_table
        self.cnn_rule, self.cnn_rules = self._conv_rule(cnn_rule, PRESETS, infer_alpha_beta, rule_table)

    def _conv_rule(self, cnn_rule, presets, infer_alpha_beta, rule_table):
        """-> (cnn_rule, cnn_rules): the (alpha, beta) of the one-rule entry and None, or None and a per-conv table
        (LRPEngine.set_cnn_rules); a table that is one alpha-beta rule with bias on every conv is that one rule"""
        names = ("alpha1beta0", "alpha2beta1")
        table = None
        if isinstance(cnn_rule, dict):                   # the keywords of LRP(...)
            if set(cnn_rule) - {"rule", "input_layer_rule"} or "rule" not in cnn_rule:
                raise ValueError("cnn_rule as a dict holds 'rule' and optionally 'input_layer_rule', the keywords of LRP(...)")
            if self.resnet is None:
                table = (cnn_rule["rule"], cnn_rule.get("input_layer_rule"))
            else:
                from .analyzer import resnet_rule_pair
                stem, units = resnet_rule_pair(cnn_rule["rule"], cnn_rule.get("input_layer_rule"))
                if stem == units and stem[0] == "alphabeta" and stem[3]:
                    return (stem[1], stem[2]), None
                return None, (stem, units)
        if isinstance(cnn_rule, str) and cnn_rule not in names:
            if cnn_rule not in presets:
                raise ValueError("cnn_rule must be (alpha, beta), 'alpha1beta0', 'alpha2beta1', one of %s or a list with a rule per conv"
                                 % sorted(presets))
            table = presets[cnn_rule]
        elif isinstance(cnn_rule, list):
            table = (cnn_rule, None)
        if table is not None:
            n_conv = len(self.cnn_cfg)
            if self.resnet is not None:
                if isinstance(cnn_rule, list):
                    raise NotImplementedError("the ResNet encoder's walk has no rule table: no list with a rule per conv")
                from .synthetic import resnet_conv_list
                n_conv = len(resnet_conv_list(self.resnet["stacks"], self.resnet.get("stem", 64)))
            table = rule_table(table[0], table[1], n_conv)
            r0 = table[0]
            if self.resnet is not None and not (r0[0] == "alphabeta" and r0[3] and all(r == r0 for r in table)):
                raise NotImplementedError("the ResNet encoder's walk is one alpha-beta rule with bias on every conv: no rule table, "
                                          "no preset %r" % (cnn_rule,))
            r0 = table[0]
            if r0[0] == "alphabeta" and r0[3] and all(r == r0 for r in table):
                return (r0[1], r0[2]), None
            return None, table
        if isinstance(cnn_rule, str):
            cnn_rule = (1, 0) if cnn_rule == "alpha1beta0" else (2, 1)
        return infer_alpha_beta(cnn_rule[0], cnn_rule[1], "CaptionModelSpec"), None


class ExplainImgCaptioningAttentionModel(object):
    _decoder_kind = None
    _applies_cnn_rule = True     # the CNN half is the LRP walk (False: the gradient baselines, whose walks ignore the rule)

    def __init__(self, model, weight_path=None, dataset_provider=None, max_caption_length=20, max_images=1,
                 device=None, layer_trace=False):
        """layer_trace=True turns the engine's trace switch on (LRPEngine.set_layer_trace): `layer_relevance` then runs."""
        if weight_path:
            with np.load(weight_path) as z:               # stands in for keras load_weights (E:27)
                model.weights.update({k: z[k] for k in z.files})
        self._model = model
        self._img_encoder = model.img_encoder
        self._dataset_provider = dataset_provider or DatasetProviderStub()
        self._preprocessor = self._dataset_provider.caption_preprocessor
        self._max_caption_length = max_caption_length
        self._hidden_dim, self._embedding_dim = model._hidden_dim, model._embedding_dim
        self.L, self.D = model.L, model.D
        self._weight_path = (weight_path or "").strip("npz")
        Tm = max_caption_length + 1
        self._engine = LRPEngine(decoder=self._decoder_kind, cnn_cfg=model.cnn_cfg, img_hw=model.img_hw, L=model.L,
                                 D=model.D, H=model._hidden_dim, E=model._embedding_dim, V=model.vocab_size,
                                 max_images=max_images, max_tokens=max_images * Tm, max_caption_len=Tm,
                                 sos_id=self._preprocessor.SOS_TOKEN_LABEL_ENCODED,
                                 eos_id=self._preprocessor.EOS_TOKEN_LABEL_ENCODED, device=device,
                                 resnet=getattr(model, "resnet", None))
        self._engine.set_weights(model.weights)
        if self._applies_cnn_rule and getattr(model, "cnn_rules", None) is not None:
            if any(r[0] == "epsilon" for r in model.cnn_rules):
                self._engine.set_precision("fp32")      # (epsilon kinds run in exact fp32 only)
            if getattr(model, "resnet", None) is not None:
                self._engine.set_resnet_rules(model.cnn_rules[1], model.cnn_rules[0])      # the pair (stem, units)
            else:
                self._engine.set_cnn_rules(model.cnn_rules)
        elif self._applies_cnn_rule and tuple(getattr(model, "cnn_rule", None) or (1, 0)) != (1, 0):
            self._engine.set_cnn_rule(*model.cnn_rule)
        self._layer_trace = bool(layer_trace)
        if self._layer_trace:
            self._engine.set_layer_trace(True)
        self._CNN_explainer = _EngineAnalyzer(self._engine)      # LRPSequentialPresetA(image_model, EPS, 'replace'), E:32
        self._state_cache = {}
        self.caption = None
        self.r_words = None

    # -------------------------------------------------------------- cached forward state as attributes
    _STATE_ATTRS = ()

    def __getattr__(self, name):
        if name.startswith("__") or name not in type(self)._STATE_ATTRS:
            raise AttributeError(name)
        if self.caption is None:
            raise AttributeError("%s is only available after _forward_beam_search" % name)
        if name not in self._state_cache:
            self._state_cache[name] = self._fetch_state(name)
        return self._state_cache[name]

    def _fetch_state(self, name):
        raise NotImplementedError()

    # -------------------------------------------------------------- protocol
    def _forward_beam_search(self, X, beam_search_captions):
        """E:370-436 / E:1092-1178: cache everything LRP needs for a given caption.
        X = (sequence_input, img_input); img_input (1,H,W,3) BGR mean-subtracted."""
        _, img_input = X
        self.caption = [int(c) for c in beam_search_captions]
        self._state_cache = {}
        self._img_input = np.asarray(img_input, dtype=np.float32)
        self._engine.encode_images(self._img_input[:1])
        self._engine.decoder_forward([self.caption])

    def _check_t(self, t):
        if self.caption is None:
            raise RuntimeError("_forward_beam_search must run first")
        if t > len(self.caption) or t < 1:
            raise NotImplementedError("index out of range of captions")          # E:538-539

    def _explain_lstm_single_word_sequence(self, t=0):
        """E:537-666 / E:1180-1321 -> (R (1,sqrtL,sqrtL,D) float32, attention_t (L,)); sets self.r_words."""
        self._check_t(t)
        R, att, rw = self._engine.decoder_explain([0], [t], variant="sequence")
        g = int(np.sqrt(self.L))
        self.r_words = self._r_words_from(rw[0].cpu().numpy(), t)
        return R.cpu().numpy().reshape(1, g, g, self.D), att[0].cpu().numpy()

    def _explain_lstm_single_word(self, t=0):
        """E:438-535 (one-step variant)."""
        self._check_t(t)
        R, att, _ = self._engine.decoder_explain([0], [t], variant="single_step", want_r_words=False)
        g = int(np.sqrt(self.L))
        return R.cpu().numpy().reshape(1, g, g, self.D), att[0].cpu().numpy()

    def _r_words_from(self, row, t):
        raise NotImplementedError()

    _batched_cnn = True      # _explain_CNN takes a stack of relevance rows (the harness then walks all words at once)

    def _explain_CNN(self, X, relevance_value, as_tensor=False):
        """E:179-181: `self._CNN_explainer.analyze([X, R])`.  The reference re-runs the whole
        encoder forward on every call (AB:511); when X is the image `_forward_beam_search`
        already encoded, the cached relevance gates are reused instead.  as_tensor=True keeps
        the (n,H,W,3) result on the device (for `engine.heatmap_render`)."""
        X = np.asarray(X, dtype=np.float32)
        R = np.asarray(relevance_value, dtype=np.float32)
        cached = getattr(self, "_img_input", None)
        if (self.caption is not None and cached is not None and X.shape[0] == 1 and X.shape == cached[:1].shape
                and np.array_equal(X, cached[:1])):
            n = R.shape[0]
            out = self._engine.cnn_explain([0] * n, R.reshape(n, self.L, self.D))
            return out if as_tensor else out.cpu().numpy()
        out = self._CNN_explainer.analyze([X, R])        # another image: the caches now belong to it
        self.caption = None
        self._state_cache = {}
        return torch.as_tensor(out).to(self._engine.device) if as_tensor else out

    def _explain_sentence(self):
        """E:183-189, but all tokens in ONE batched launch chain."""
        n = len(self.caption) - 1
        ts = list(range(1, n + 1))
        R, att, rw = self._engine.decoder_explain([0] * n, ts, variant="sequence")
        g = int(np.sqrt(self.L))
        Rn = R.cpu().numpy()
        if n:
            self.r_words = self._r_words_from(rw[n - 1].cpu().numpy(), n)
        rel = [Rn[i].reshape(1, g, g, self.D) for i in range(n)]
        return rel, self.attention[1:-1]

    def layer_relevance(self, ts=None, keep=()):
        """The relevance at every layer's input of the CNN walk, for the words `ts` (default: all) of the caption last forwarded:
        the reverse analyzers' reverse_keep_tensors / reverse_check_* output (innvestigate/analyzer/base.py:570-603) per word.
        Returns (ids, stats, kept): ids [(nid, 0)] sorted — (-1, 0) the head R_feat, (0, 0) the image; stats
        (n_words, n_tensors, 4) float64 numpy — minimum, maximum, sum, non-finite count; kept: dict id -> (n_words, H, W, C)
        float32 tensor for the ids in `keep` (True: all).  Needs layer_trace=True at construction."""
        if not self._layer_trace:
            raise RuntimeError("layer_relevance needs the trace switch: construct the explainer with layer_trace=True")
        if self.caption is None:
            raise RuntimeError("_forward_beam_search must run first")
        ts = list(range(1, len(self.caption))) if ts is None else [int(t) for t in ts]
        for t in ts:
            self._check_t(t)
        n = len(ts)
        R, _, _ = self._engine.decoder_explain([0] * n, ts, variant="sequence", want_attention=False, want_r_words=False)
        _, stats, kept = self._engine.cnn_explain_traced([0] * n, R, keep=keep)
        ids = [i for i, _ in self._engine.trace_tensors()]
        return ids, stats.permute(1, 0, 2).cpu().numpy(), kept

    # -------------------------------------------------------------- batched entry points (new)
    def explain_batch(self, images, captions, return_R_feat=False):
        """images (B,H,W,3), captions: list of id lists ending in EOS.  Returns
        (R_img (sum_b T_b, H, W, 3) torch tensor on the GPU, index list [(b, t)], attention, r_words)."""
        self._engine.encode_images(images)
        self._engine.decoder_forward(captions)
        pairs = [(b, t) for b, c in enumerate(captions) for t in range(1, len(c))]
        out, R, att, rw = self._engine.explain_tokens([p[0] for p in pairs], [p[1] for p in pairs],
                                                      want_R_feat=return_R_feat, want_attention=True, want_r_words=True)
        return out, pairs, att, rw, R

    device_search = False      # True: `_beam_search` keeps the beam bookkeeping on the device too (`on_device=None` reads this)

    def _beam_search(self, X, beam_size=3, on_device=None):
        """Caption generation (E:51-120; the batched form of inference.py:178-253).  Upstream of the LRP path (captions
        are an input to it); provided so harnesses run end to end.
          * bookkeeping = `beam.search`: the reference's two bounded heaps, EOS handling and final pick, pinned against
            the reference's own `_beam_search` on canned scores (tests/test_beam.py);
          * scores: the hypotheses' decoder state stays on the device (lrp_decoder_gen_begin / _gen_step: one decoder
            step per search step for ALL beams of ALL images that fit the handle — max_images >= images x beam_size —
            where the reference re-runs the whole captioner on every partial caption, E:71), and so does the ranking
            (lrp_op_log_softmax_topk): per step only beam_size (id, log p) pairs per hypothesis come to the host.
        on_device=True (default: the class attribute `device_search`) moves the bookkeeping to the device as well
        (`LRPEngine.beam_search`: all steps of a group enqueued at once, one copy of the results per group); the captions
        are the same lists (tests/test_gpu_beam_device.py).
        Returns, per image, up to beam_size captions, element [0] = the reference's answer (one image: that list)."""
        from . import beam
        if on_device is None:
            on_device = self.device_search
        _, imgs_input = X
        imgs_input = np.asarray(imgs_input, dtype=np.float32)
        EOS = self._preprocessor.EOS_TOKEN_LABEL_ENCODED
        eng = self._engine
        k = beam_size
        if k > eng.max_images:
            return self._beam_search_replay(X, beam_size)          # not enough feature slots for one row per beam
        results = []
        group = max(1, eng.max_images // k)      # images searched together: one decoder step serves all their beams
        for lo in range(0, len(imgs_input), group):
            imgs = imgs_input[lo:lo + group]
            G = len(imgs)
            eng.encode_images(imgs)
            feat = eng.get_features()[:G]
            eng.set_features(feat.repeat_interleave(k, dim=0).contiguous())    # one row (feature slot) per (image, beam)
            eng.gen_begin(G * k)
            if on_device:
                results += eng.beam_search_lists(G, k, self._max_caption_length, EOS)
                continue

            def step(s, parent, word):
                logits = eng.gen_step(s, parent, word)                          # (G * k, V) float64, stays on the device
                ids, logp = eng.log_softmax_topk(logits, k)
                return ids.cpu().numpy(), logp.cpu().numpy()
            results += beam.search(step, G, k, self._max_caption_length, EOS)
        self.caption = None
        self._state_cache = {}
        return results[0] if len(results) == 1 else results

    def _beam_search_replay(self, X, beam_size=3):
        """The same search with the scores taken from the teacher-forced decoder replay (every step re-plays the live
        hypotheses from scratch, like the reference's predict_on_batch loop) and ranked on the host: the cross-check of
        `_beam_search`'s incremental device state and device-side ranking."""
        from . import beam
        _, imgs_input = X
        imgs_input = np.asarray(imgs_input, dtype=np.float32)
        EOS = self._preprocessor.EOS_TOKEN_LABEL_ENCODED
        eng = self._engine
        k = beam_size
        results = []
        for img in imgs_input:
            eng.encode_images(img[None])
            hist = {}

            def step(s, parent, word):
                nonlocal hist
                hist = {r: [] for r in range(k)} if s == 0 else {r: hist[parent[r]] + [int(word[r])] for r in range(k)}
                rows = []
                for r in range(k):
                    eng.decoder_forward([hist[r] + [EOS]])
                    rows.append(eng.read_state("caption_preds")[0, s].cpu().numpy())
                return beam.topk_log_softmax(np.stack(rows), k)
            results += beam.search(step, 1, k, self._max_caption_length, EOS)
        self.caption = None
        self._state_cache = {}
        return results[0] if len(results) == 1 else results


class _EngineAnalyzer(object):
    """`analyze([X, R])` of LRPSequentialPresetA (AB:478-520) on an engine's encoder."""

    def __init__(self, engine):
        self._engine = engine

    def analyze(self, X):
        X = list(X) if isinstance(X, (list, tuple)) else [X]
        if len(X) != 2:
            raise ValueError("neuron_selection_mode 'replace' expects [X, R]")
        img, R = np.asarray(X[0], dtype=np.float32), np.asarray(X[1], dtype=np.float32)
        n = img.shape[0]
        if R.shape[0] != n:
            raise ValueError("X and R must have the same batch size")
        e = self._engine
        out = np.empty_like(img)
        for lo in range(0, n, e.max_images):
            hi = min(n, lo + e.max_images, lo + e.max_tokens)
            e.encode_images(img[lo:hi])
            out[lo:hi] = e.cnn_explain(list(range(hi - lo)), R[lo:hi].reshape(hi - lo, e.L, e.D)).cpu().numpy()
        return out


class ExplainImgCaptioningAdaptiveAttention(ExplainImgCaptioningAttentionModel):
    """E:260-666."""
    _decoder_kind = "adaptive"
    _STATE_ATTRS = ("ht", "ct", "gt", "it_act", "ft_act", "context", "attention", "st", "beta", "c_hat", "xt",
                    "caption_preds", "_image_features_before_act", "_average_img_feature",
                    "_global_img_feature_before_act", "_total_static_img_feature", "_img_feature_input")
    _ENGINE_NAME = {"_image_features_before_act": "image_features_before_act",
                    "_average_img_feature": "average_img_feature",
                    "_global_img_feature_before_act": "global_img_feature_before_act",
                    "_total_static_img_feature": "total_static_img_feature"}

    def _fetch_state(self, name):
        n = len(self.caption)
        if name == "_img_feature_input":
            return self._engine.get_features()[0].cpu().numpy()
        a = self._engine.read_state(self._ENGINE_NAME.get(name, name))[0].cpu().numpy()
        if name in ("xt", "caption_preds"):
            return a[:n]
        if name.startswith("_"):
            return a[0] if a.shape[0] == 1 else a
        return a[:n + 1]                              # row 0 = zero init (E:389-398)

    def _r_words_from(self, row, t):
        return row[:t - 1]                            # normalised, first dropped (E:660-665)


class ExplainImgCaptioningGridTDModel(ExplainImgCaptioningAttentionModel):
    """E:995-1321."""
    _decoder_kind = "gridtd"
    _STATE_ATTRS = ("h1t", "c1t", "g1t", "i1t_act", "f1t_act", "h2t", "c2t", "g2t", "i2t_act", "f2t_act", "x1t", "x2t",
                    "context", "st", "beta", "context_hat", "attention", "caption_preds")

    def _fetch_state(self, name):
        n = len(self.caption)
        a = self._engine.read_state(name)[0].cpu().numpy()
        if name in ("x1t", "x2t", "caption_preds"):
            return a[:n]
        return a[:n + 1]

    def _r_words_from(self, row, t):
        return row[:t]                                # un-normalised (E:1320)

    def _explain_lstm_single_word(self, t=0):
        raise NotImplementedError()                   # E:167-172: the grid-TD class does not override it


# ---------------------------------------------------------------------------------------------------------------
# Gradient baselines: the reference's six comparison engines on the same cached forward.
# Decoder half = its hand-written BPTT `_lstm_decoder_backward` (lrp_decoder_gradient); CNN half = iNNvestigate's
# Gradient / InputTimesGradient / GuidedBackprop with neuron_selection_mode="replace" (lrp_cnn_walk).
# ---------------------------------------------------------------------------------------------------------------
class _GradientMixin(object):
    _walk = "gradient"
    _applies_cnn_rule = False

    def __init__(self, *args, **kwargs):
        super(_GradientMixin, self).__init__(*args, **kwargs)
        # A gradient through ReLUs / max-pools switches whole paths where a pre-activation is zero to the forward's own
        # accuracy (LRP does not: such a unit carries ~ 0 relevance).  The comparison baselines therefore run the engine
        # with the forward that takes the fewest of those decisions differently from float64 — the exact fp32 MFMA
        # (their walks are exact fp32 in every mode): VGG16-size gradient maps 7e-7 from float64 instead of ~1e-3
        # (tests/test_gpu_gradient.py).  `self._engine.set_precision("bf16x3")` restores the faster default forward on a VGG
        # encoder; a ResNet encoder's gradient walks exist in this mode only (include/lrp_hip.h, lrp_cnn_walk).
        self._engine.set_precision("fp32")

    def _lstm_decoder_backward(self, t):
        """E:780-832 / E:1452-1532 -> d_img_feature (1, sqrtL, sqrtL, D) float32; sets self.r_words (t,).
        Adaptive decoder with embedding_dim != hidden_dim: NotImplementedError (the reference's class raises there,
        E:798 / E:823; lrp_decoder_gradient returns LRP_ERR_UNSUPPORTED).  The grid-TD classes run at any E % 4 == 0."""
        self._check_t(t)
        d, rw = self._engine.decoder_gradient([0], [t])
        g = int(np.sqrt(self.L))
        self.r_words = rw[0, :t].cpu().numpy()
        return d.cpu().numpy().reshape(1, g, g, self.D)

    def _explain_sentence(self):
        """E:834-839 / E:1534-1539: a list of relevances only (no attention), all words in one batched call."""
        n = len(self.caption) - 1
        if n < 1:
            return []
        d, rw = self._engine.decoder_gradient([0] * n, list(range(1, n + 1)))
        g = int(np.sqrt(self.L))
        self.r_words = rw[n - 1, :n].cpu().numpy()
        dn = d.cpu().numpy()
        return [dn[i].reshape(1, g, g, self.D) for i in range(n)]

    def _explain_CNN(self, X, relevance_value, as_tensor=False):
        """`self._CNN_explainer.analyze([X, relevance])` with the class's analyzer (E:672 / :884 / :928)."""
        X = np.asarray(X, dtype=np.float32)
        R = np.asarray(relevance_value, dtype=np.float32)
        cached = getattr(self, "_img_input", None)
        if not (self.caption is not None and cached is not None and X.shape == cached[:1].shape and np.array_equal(X, cached[:1])):
            self._engine.encode_images(X[:1])              # another image: the caches now belong to it
            self._img_input = X[:1].copy()
            self.caption = None
            self._state_cache = {}
        n = R.shape[0]
        out = self._engine.cnn_walk([0] * n, R.reshape(n, self.L, self.D), self._walk)
        return out if as_tensor else out.cpu().numpy()

    def layer_relevance(self, ts=None, keep=()):
        raise NotImplementedError("the layer trace is built for the LRP walk only, not for the gradient-family walks")

    def _explain_lstm_single_word_sequence(self, t=0):
        raise NotImplementedError("the gradient engines explain through _lstm_decoder_backward")   # E:174-177 base stub

    def _explain_lstm_single_word(self, t=0):
        raise NotImplementedError("the gradient engines explain through _lstm_decoder_backward")


class _GuidedGradcamMixin(_GradientMixin):
    _walk = "guided_backprop"
    _batched_cnn = False     # the Grad-CAM factor is per word (E:930-937)

    def grad_cam(self, img_feature, grads):
        from .postprocess import grad_cam
        return grad_cam(img_feature, grads, self.L, self.D, upscale=self._model.img_hw[0] // int(np.sqrt(self.L)))

    def _explain_CNN(self, X, relevance_value):
        """E:930-937 / E:1634-1641: guided backprop of the image model, gated by the Grad-CAM map of the features."""
        R = np.asarray(relevance_value, dtype=np.float32)
        gb = _GradientMixin._explain_CNN(self, X, R)
        feat = self._engine.get_features()[0].cpu().numpy()
        cam = self.grad_cam(feat, R[0])
        return (gb[0] * cam[..., np.newaxis])[np.newaxis, :]

    # -------------------------------------------------------------- batched forms on the device (new; lrp_op_gradcam)
    def grad_cam_device(self, grads):
        """`grad_cam` of n gradient rows of the cached image at once, in fp64 on the device: grads (n, L, D) or
        (n, g, g, D) -> (n, S, S) float64 tensor."""
        from .engine import op_gradcam
        g = int(np.sqrt(self.L))
        d = self._engine._dev(grads).reshape(-1, self.L, self.D)
        return op_gradcam(self._engine.get_features()[:1], [0] * d.shape[0], d, g, self._model.img_hw[0] // g)

    def explain_words(self, ts, want_cam=False):
        """`_explain_CNN(X, _lstm_decoder_backward(t))` for every t of `ts` in one chain on the cached caption:
        (len(ts), H, W, 3) float64 tensor on the device (and the cams on request)."""
        ts = [int(t) for t in ts]
        for t in ts:
            self._check_t(t)
        return self._engine.guided_gradcam([0] * len(ts), ts, want_cam=want_cam)

    def explain_sentence_cnn(self):
        """Every word of the cached caption: explain_words(1 .. len(caption) - 1)."""
        if self.caption is None:
            raise RuntimeError("_forward_beam_search must run first")
        return self.explain_words(range(1, len(self.caption)))


class ExplainImgCaptioningAdaptiveAttentionGradient(_GradientMixin, ExplainImgCaptioningAdaptiveAttention):
    """E:667-879."""
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningAdaptiveAttentionInputTimesGradient(ExplainImgCaptioningAdaptiveAttentionGradient):
    """E:880-924."""
    _walk = "input_x_gradient"


class ExplainImgCaptioningAdaptiveAttentionGuidedGradcam(_GuidedGradcamMixin, ExplainImgCaptioningAdaptiveAttention):
    """E:925-993."""
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningGridTDGradient(_GradientMixin, ExplainImgCaptioningGridTDModel):
    """E:1322-1583."""
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


class ExplainImgCaptioningGridTDGradientTimesInput(ExplainImgCaptioningGridTDGradient):
    """E:1584-1628."""
    _walk = "input_x_gradient"


class ExplainImgCaptioningGridTDGuidedGradcam(_GuidedGradcamMixin, ExplainImgCaptioningGridTDModel):
    """E:1629-1700 (its guided_backproe helper, E:1655-1657, is `_explain_CNN` without the Grad-CAM factor)."""
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")

    def guided_backproe(self, img_input, grads):
        return _GradientMixin._explain_CNN(self, img_input, grads)


# ---------------------------------------------------------------------------------------------------------------
# Deconvnet, SmoothGrad and IntegratedGradients (innvestigate/analyzer/gradient_based.py:180-225, :273-319) as comparison engines
# in the shape of the six above: decoder half = `_lstm_decoder_backward`, unchanged; CNN half = the analyzer named.  The reference
# has no such classes (its wrappers cannot run with a replaced head, wrapper.py:84-86); the names follow its scheme.
# ---------------------------------------------------------------------------------------------------------------
class _DeconvnetMixin(_GradientMixin):
    _walk = "deconvnet"


class _DeepLIFTMixin(_GradientMixin):
    """CNN half = analyzer.DeepLIFT (deeplift.py:44-250) on the explainer's own engine: the 'deeplift' walk against the forward of
    `reference_inputs` (a scalar or an array that broadcasts to (1, H, W, 3)); VGG-style encoders, exact fp32."""
    _walk = "deeplift"

    def __init__(self, *args, **kwargs):
        reference_inputs = kwargs.pop("reference_inputs", 0)
        approximate_gradient = bool(kwargs.pop("approximate_gradient", True))
        super(_DeepLIFTMixin, self).__init__(*args, **kwargs)
        from .analyzer import check_deeplift_reference
        self._engine.set_deeplift_reference(check_deeplift_reference(reference_inputs, self._model.img_hw), approximate_gradient)


class _AugmentedMixin(_GradientMixin):
    """`_explain_CNN(X, R)` on an analyzer instance of its own, created on first use from an ImageModelSpec of the model's encoder
    weights: a second, CNN-only handle, as every analyzer of analyzer.py has.  The explainer's own engine — its encode caches
    and the decoder state of `_forward_beam_search` — is not touched by it."""
    _analyzer_name = None
    _batched_cnn = False     # one (image, head) per call: the samples of a word fill the analyzer's batch
    _KW = ()

    def __init__(self, *args, **kwargs):
        self._analyzer_kwargs = {k: kwargs.pop(k) for k in self._KW + ("max_batch", "postprocess") if k in kwargs}
        super(_AugmentedMixin, self).__init__(*args, **kwargs)
        self._augmented = None

    def _cnn_analyzer(self):
        if self._augmented is None:
            from . import analyzer as A
            m = self._model
            spec = A.ImageModelSpec(m.weights, cnn_cfg=m.cnn_cfg, img_hw=m.img_hw, resnet=getattr(m, "resnet", None))
            self._augmented = getattr(A, self._analyzer_name)(spec, device=self._engine.device.index, **self._analyzer_kwargs)
        return self._augmented

    def _explain_CNN(self, X, relevance_value, as_tensor=False):
        X = np.asarray(X, dtype=np.float32)
        R = np.asarray(relevance_value, dtype=np.float32)
        n = R.shape[0]
        out = self._cnn_analyzer().analyze([np.repeat(X[:1], n, axis=0), R.reshape((n,) + tuple(R.shape[1:]))])
        return torch.as_tensor(out).to(self._engine.device) if as_tensor else out


class _SmoothGradMixin(_AugmentedMixin):
    _analyzer_name = "SmoothGrad"
    _KW = ("augment_by_n", "noise_scale", "seed")


class _IntegratedGradientsMixin(_AugmentedMixin):
    _analyzer_name = "IntegratedGradients"
    _KW = ("steps", "reference_inputs", "path")


class ExplainImgCaptioningAdaptiveAttentionDeconvnet(_DeconvnetMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningAdaptiveAttentionSmoothGrad(_SmoothGradMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningAdaptiveAttentionIntegratedGradients(_IntegratedGradientsMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningGridTDDeconvnet(_DeconvnetMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


class ExplainImgCaptioningGridTDSmoothGrad(_SmoothGradMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


class ExplainImgCaptioningGridTDIntegratedGradients(_IntegratedGradientsMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")



class ExplainImgCaptioningAdaptiveAttentionDeepLIFT(_DeepLIFTMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningGridTDDeepLIFT(_DeepLIFTMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


# ---------------------------------------------------------------------------------------------------------------
# PatternNet / PatternAttribution (innvestigate/analyzer/pattern_based.py:128-281) as comparison engines, as the DeepLIFT pair:
# decoder half = `_lstm_decoder_backward`; CNN half = the 'patternnet' / 'pattern_attribution' walk of the explainer's own engine
# on the patterns given at construction (`patterns=`, one HWIO array per conv) or fitted by `fit_patterns(images)`.
# ---------------------------------------------------------------------------------------------------------------
class _PatternNetMixin(_GradientMixin):
    _walk = "patternnet"

    def __init__(self, *args, **kwargs):
        patterns = kwargs.pop("patterns", None)
        self._pattern_type = kwargs.pop("pattern_type", None)
        project = kwargs.pop("reverse_project_bottleneck_layers", True)
        super(_PatternNetMixin, self).__init__(*args, **kwargs)
        if getattr(self._model, "resnet", None) is not None:
            raise NotImplementedError("PatternNet is built for the VGG-style (conv-list) encoders only")
        self._engine.set_pattern_projection(project)
        self._has_patterns = patterns is not None
        if self._has_patterns:
            self._engine.set_patterns(list(patterns))

    def fit_patterns(self, images, batch_size=32):
        """Fit the patterns on `images` (N, H, W, 3) with the explainer's own engine (LRPEngine.pattern_fit).  The encode caches
        then belong to the last batch: the cached caption and image are dropped."""
        pattern_type = "relu" if self._pattern_type is None else self._pattern_type
        if isinstance(pattern_type, (list, tuple)):
            raise ValueError("Only one pattern type allowed. Please pass a string.")
        self._engine.pattern_fit(images, pattern_type, batch=batch_size)
        self._has_patterns = True
        self._img_input = None
        self.caption = None
        self._state_cache = {}
        return self._engine.get_patterns()

    def _explain_CNN(self, X, relevance_value, as_tensor=False):
        if not self._has_patterns:
            raise RuntimeError("no patterns: pass patterns= or call fit_patterns(images) first")
        return super(_PatternNetMixin, self)._explain_CNN(X, relevance_value, as_tensor=as_tensor)


class _PatternAttributionMixin(_PatternNetMixin):
    _walk = "pattern_attribution"


class ExplainImgCaptioningAdaptiveAttentionPatternNet(_PatternNetMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningAdaptiveAttentionPatternAttribution(_PatternAttributionMixin, ExplainImgCaptioningAdaptiveAttention):
    _STATE_ATTRS = ExplainImgCaptioningAdaptiveAttention._STATE_ATTRS + ("ot_act",)


class ExplainImgCaptioningGridTDPatternNet(_PatternNetMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


class ExplainImgCaptioningGridTDPatternAttribution(_PatternAttributionMixin, ExplainImgCaptioningGridTDModel):
    _STATE_ATTRS = ExplainImgCaptioningGridTDModel._STATE_ATTRS + ("o1t_act", "o2t_act")


# ---------------------------------------------------------------------------------------------------------------
# Occlusion sensitivity and RISE (saliency.py): the model-agnostic controls.  Nothing is walked backwards and nothing
# encoder-specific is read, so the classes run on VGG-style and ResNet specs alike.  The reference has no such classes; the names
# follow its scheme.  Constructor keywords of the driver (OcclusionSaliency / RISESaliency) are forwarded to it.
# ---------------------------------------------------------------------------------------------------------------
class _SaliencyMixin(object):
    _driver = None           # the driver class of saliency.py
    _KW = ()
    _applies_cnn_rule = False

    def __init__(self, *args, **kwargs):
        from . import saliency
        driver = getattr(saliency, self._driver)
        kw = {k: kwargs.pop(k) for k in self._KW if k in kwargs}
        driver.check_arguments(**kw)                           # (before an engine is created)
        super(_SaliencyMixin, self).__init__(*args, **kwargs)
        self._saliency = driver(self, **kw)

    def explain_images(self, images, captions=None, words=None):
        """The driver's `explain`: {"units": [(image, t)], "maps": (n_units, H, W) float32 device tensor, "scores0": ...}."""
        return self._saliency.explain(images, captions, words)

    def _no_walk(self, *args, **kwargs):
        raise NotImplementedError("occlusion, RISE, LIME and KernelSHAP explain whole images through explain_images: there is no "
                                  "decoder or CNN walk")

    _explain_lstm_single_word_sequence = _explain_lstm_single_word = _explain_CNN = _explain_sentence = layer_relevance = _no_walk


class _OcclusionMixin(_SaliencyMixin):
    _driver = "OcclusionSaliency"
    _KW = ("window", "stride", "fill", "score")


class _RISEMixin(_SaliencyMixin):
    _driver = "RISESaliency"
    _KW = ("n_masks", "s", "p", "seed", "fill", "score", "keys")


class ExplainImgCaptioningAdaptiveAttentionOcclusion(_OcclusionMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningAdaptiveAttentionRISE(_RISEMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningGridTDOcclusion(_OcclusionMixin, ExplainImgCaptioningGridTDModel):
    pass


class ExplainImgCaptioningGridTDRISE(_RISEMixin, ExplainImgCaptioningGridTDModel):
    pass


# LIME and KernelSHAP (saliency.py): the same scheme; `segments` is a (B, H, W) int label map from any segmenter of the caller's
# (None: the regular grid of the `cells` keyword)
class _SegmentMixin(_SaliencyMixin):
    def explain_images(self, images, captions=None, words=None, segments=None):
        """The driver's `explain`: the keys above, plus "coefficients", "intercept", "segments" and "status"."""
        return self._saliency.explain(images, captions, words, segments)


class _LIMEMixin(_SegmentMixin):
    _driver = "LIMESaliency"
    _KW = ("n_samples", "cells", "p", "kernel_width", "ridge", "seed", "fill", "score", "keys")


class _KernelSHAPMixin(_SegmentMixin):
    _driver = "KernelSHAPSaliency"
    _KW = ("n_samples", "cells", "ridge", "seed", "fill", "score", "keys")


class ExplainImgCaptioningAdaptiveAttentionLIME(_LIMEMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningAdaptiveAttentionKernelSHAP(_KernelSHAPMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningGridTDLIME(_LIMEMixin, ExplainImgCaptioningGridTDModel):
    pass


class ExplainImgCaptioningGridTDKernelSHAP(_KernelSHAPMixin, ExplainImgCaptioningGridTDModel):
    pass


# The CAM family (saliency.py; csrc/cam_kernels.h): the same scheme.  CAM takes method= ('gradcam', 'gradcam++', 'xgradcam',
# 'layercam', 'hirescam') and guided=; it reads the decoder gradient and is limited as the gradient baselines above are (exact
# fp32 forward; adaptive decoder with embedding_dim == hidden_dim).  ScoreCAM and AblationCAM read forwards only.  The Guided
# Grad-CAM classes above are the reference's and stay as they are.
class _CAMMixin(_SaliencyMixin):
    _driver = "GradientCAMSaliency"
    _KW = ("method", "guided")


class _ScoreCAMMixin(_SaliencyMixin):
    _driver = "ScoreCAMSaliency"
    _KW = ("weights", "fill", "score")


class _AblationCAMMixin(_SaliencyMixin):
    _driver = "AblationCAMSaliency"
    _KW = ("score",)


class ExplainImgCaptioningAdaptiveAttentionCAM(_CAMMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningAdaptiveAttentionScoreCAM(_ScoreCAMMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningAdaptiveAttentionAblationCAM(_AblationCAMMixin, ExplainImgCaptioningAdaptiveAttention):
    pass


class ExplainImgCaptioningGridTDCAM(_CAMMixin, ExplainImgCaptioningGridTDModel):
    pass


class ExplainImgCaptioningGridTDScoreCAM(_ScoreCAMMixin, ExplainImgCaptioningGridTDModel):
    pass


class ExplainImgCaptioningGridTDAblationCAM(_AblationCAMMixin, ExplainImgCaptioningGridTDModel):
    pass
