"""`LRPSequentialPresetA` with the iNNvestigate call surface the captioning code uses
(innvestigate/analyzer/relevance_based/relevance_analyzer.py:695-721, base.py:328-347, :478-520):

    analyzer = LRPSequentialPresetA(image_model, epsilon=0.01, neuron_selection_mode='replace')
    relevance = analyzer.analyze([X, R])          # X (N,224,224,3), R (N,14,14,512) -> (N,224,224,3)

`image_model` is an `ImageModelSpec` (layer list + weights) instead of a Keras model: the
symbolic graph reversal of the reference (utils/keras/graph.py:704-942) is not reproduced,
only its semantics — Conv -> Alpha1Beta0Rule, MaxPooling -> gradient routing, fused ReLU ->
pass-through, head relevance := second input — executed by the HIP encoder path.

The gradient baselines beside it (innvestigate/analyzer/gradient_based.py:101-265), same surface:

    Gradient(image_model, postprocess=None | "abs" | "square", neuron_selection_mode='replace')
    InputTimesGradient(image_model, ...)          # gradient (post-processed) x X
    GuidedBackprop(image_model, ...)              # every ReLU clamps what arrives at 0 before its own gradient
    analyzer.analyze([X, head])                   # -> (N,H,W,3)

on lrp_cnn_walk in exact fp32 (LRP_PREC_FP32: a ReLU decision taken in another arithmetic switches whole gradient paths),
for a VGG-style or a ResNet `ImageModelSpec`.

And the rest of the gradient-based entries that need no trained side data (gradient_based.py:180-225, :273-319; wrapper.py:214-345):

    Deconvnet(image_model)                        # every ReLU clamps what arrives at 0 and passes it on: no forward decision is read
    GaussianSmoother(subanalyzer, augment_by_n=2, noise_scale=1, seed=0)
    PathIntegrator(subanalyzer, steps=16, reference_inputs=0, path="reference" | "standard")
    SmoothGrad(image_model, augment_by_n=64, postprocess=None, ...)       # GaussianSmoother over Gradient
    IntegratedGradients(image_model, steps=64, postprocess=None, ...)     # PathIntegrator over Gradient

with samples, walks and the mean on the device (LRPEngine.cnn_walk_augmented); `analyzers` maps the reference's names to what is built.

DeepLIFT and DeepTaylor (innvestigate/analyzer/deeplift.py:44-250, deeptaylor.py:40-199), VGG-style encoders, reached by name:

    DeepLIFT(image_model, reference_inputs=0, approximate_gradient=True)    # LRPEngine.set_deeplift_reference + the 'deeplift' walk
    DeepTaylor(image_model) / BoundedDeepTaylor(image_model, low, high)     # the default walk / the bounded table, head [feat > 0]

PatternNet and PatternAttribution (pattern_based.py:128-281), VGG-style encoders, reached by name as well:

    PatternNet(image_model, patterns=None, pattern_type=None)               # .fit(X) / .fit_generator(gen) or patterns from
    PatternAttribution(image_model, patterns=None, pattern_type=None)       # pattern.PatternComputer; the 'patternnet' / 'pattern_attribution' walks
"""
import numpy as np

from .engine import LRPEngine
from .explainers import _EngineAnalyzer
from .synthetic import VGG16_CFG


class NotAnalyzeableModelException(Exception):
    """innvestigate/analyzer/base.py:37-39."""


class ImageModelSpec(object):
    """The truncated encoder `Model(input_1 -> block5_conv3)` (explainers.py:29-30) as data: a VGG-style conv list,
    or (resnet=dict(stem, stacks)) the ResNet-v1 bottleneck stack cut at conv5_block3_out.  The analyzer's head
    shape follows from it — (14,14,512) / (7,7,2048) in the reference's hard-coded table (base.py:370-373)."""

    def __init__(self, weights, cnn_cfg=VGG16_CFG, img_hw=(224, 224), resnet=None):
        self.img_hw = tuple(img_hw)
        self.resnet = resnet
        if resnet is None:
            self.cnn_cfg = list(cnn_cfg)
            self.weights = {k: v for k, v in weights.items() if k.endswith(("_W", "_b")) and k[:-2] in {c[0] for c in cnn_cfg}}
            missing = [c[0] for c in cnn_cfg if c[0] + "_W" not in self.weights or c[0] + "_b" not in self.weights]
        else:
            from .synthetic import resnet_conv_list
            self.cnn_cfg = VGG16_CFG
            names = [c[0] for c in resnet_conv_list(resnet["stacks"], resnet.get("stem", 64))]
            sufs = ("_conv_W", "_conv_b", "_bn_gamma", "_bn_beta", "_bn_mean", "_bn_var")
            self.weights = {n + s: weights[n + s] for n in names for s in sufs if n + s in weights}
            missing = [n + s for n in names for s in sufs if n + s not in weights]
        if missing:
            raise NotAnalyzeableModelException("weights missing for layers %s" % missing[:8])

    def output_shape(self):
        h, w = self.img_hw
        if self.resnet is not None:
            stacks = self.resnet["stacks"]
            d = 4 * 2 ** (len(stacks) - 1)
            return h // d, w // d, 4 * stacks[-1][0]
        for _, _, _, pool in self.cnn_cfg:
            if pool:
                h, w = h // 2, w // 2
        return h, w, self.cnn_cfg[-1][2]


def reversed_tensor_ids(cnn_cfg):
    """The sorted ids of the reversed tensors of a VGG-style conv list (base.py:715-802; graph.py:770-816): (-1, 0) the head,
    (nid, 0) the relevance at the input of node nid — the convs and 2x2 pools in execution order."""
    n_nodes = sum(2 if pool else 1 for _, _, _, pool in cnn_cfg)
    return [(nid, 0) for nid in range(-1, n_nodes)]


class LRPSequentialPresetA(object):
    """analyze([X, R]) on the engine's LRP walk.  The reverse analyzers' inspection switches (base.py:570-603) are taken by name on
    a VGG-style spec — reverse_keep_tensors, reverse_check_min_max_values, reverse_check_finite: with any of them set, analyze runs
    the traced walk (LRPEngine.cnn_explain_traced), prints the reference's lines (base.py:769-802) and sets `_reversed_tensors`,
    the sorted list of ((nid, 0), float32 ndarray (N, H, W, C)), as the reference does, and `_reversed_stats`, a dict
    id -> {"min", "max", "sum" (per input row), "nonfinite"}.  The ids: (-1, 0) the head, (nid, 0) the relevance at the input of
    node nid (convs and 2x2 pools in execution order).  reverse_clip_values and reverse_project_bottleneck_layers change the walk
    itself and are not built."""

    def __init__(self, model, epsilon=0.1, neuron_selection_mode="replace", max_batch=8, device=None, reverse_keep_tensors=False,
                 reverse_check_min_max_values=False, reverse_check_finite=False, reverse_clip_values=False,
                 reverse_project_bottleneck_layers=False, **kwargs):
        if neuron_selection_mode not in ["max_activation", "index", "all", "replace"]:
            raise ValueError("neuron_selection parameter is not valid.")             # base.py:332-333
        if neuron_selection_mode != "replace":
            raise NotImplementedError("only neuron_selection_mode='replace' is on the captioning hot path")
        if not (epsilon > 0):
            raise ValueError("epsilon must be > 0")                                   # relevance_based/utils.py:52-60
        if reverse_clip_values or reverse_project_bottleneck_layers:
            raise NotImplementedError("reverse_clip_values and reverse_project_bottleneck_layers change the walk itself and are not built")
        self._reverse_keep_tensors = bool(reverse_keep_tensors)
        self._reverse_check_min_max_values = bool(reverse_check_min_max_values)
        self._reverse_check_finite = bool(reverse_check_finite)
        self._trace = self._reverse_keep_tensors or self._reverse_check_min_max_values or self._reverse_check_finite
        if self._trace and getattr(model, "resnet", None) is not None:
            raise NotImplementedError("the reverse_* inspection switches are built for the VGG-style (conv-list) encoders only")
        self._epsilon = epsilon          # used by Dense layers only (PresetA); the truncated encoders have none
        self._neuron_selection_mode = neuron_selection_mode
        self._model = model
        h, w, c = model.output_shape()
        # the decoder half of the handle is idle here: minimal dims (lrp_create: H a multiple of 8)
        self._engine = LRPEngine(decoder="adaptive", cnn_cfg=model.cnn_cfg, img_hw=model.img_hw, L=h * w, D=c, H=8, E=8,
                                 V=4, max_images=max_batch, max_tokens=max_batch, max_caption_len=2, device=device,
                                 resnet=model.resnet)
        self._engine.set_weights(model.weights)
        if self._trace:
            self._engine.set_layer_trace(True)
        self._impl = _EngineAnalyzer(self._engine)

    def analyze(self, X, neuron_selection=None):
        if neuron_selection is not None:
            raise ValueError("Only neuron_selection_mode 'index' expects the neuron_selection parameter.")  # base.py:489-492
        if self._trace:
            return self._analyze_traced(X)
        return self._impl.analyze(X)

    def reversed_tensor_ids(self):
        """The ids of the reversed tensors, sorted: (-1, 0), (0, 0), ... (N - 1, 0) for the N convs and pools of the spec."""
        return reversed_tensor_ids(self._model.cnn_cfg)

    def _analyze_traced(self, X, mask_head=False):
        """analyze through the traced walk, in chunks of max_batch; mask_head: head [feat > 0] first (DeepTaylor)."""
        X = list(X) if isinstance(X, (list, tuple)) else [X]
        if len(X) != 2:
            raise ValueError("neuron_selection_mode 'replace' expects [X, R]")
        img, R = np.asarray(X[0], dtype=np.float32), np.asarray(X[1], dtype=np.float32)
        n = img.shape[0]
        if R.shape[0] != n:
            raise ValueError("X and R must have the same batch size")
        e = self._engine
        ids = [i for i, _ in e.trace_tensors()]
        out = np.empty_like(img)
        stats, parts = [], dict((i, []) for i in ids)
        for lo in range(0, n, e.max_images):
            hi = min(n, lo + e.max_images, lo + e.max_tokens)
            e.encode_images(img[lo:hi])
            head = R[lo:hi].reshape(hi - lo, e.L, e.D)
            if mask_head:
                head = head * (e.get_features()[:hi - lo].cpu().numpy() > 0)
            r, st, kept = e.cnn_explain_traced(list(range(hi - lo)), head, keep=True if self._reverse_keep_tensors else ())
            out[lo:hi] = r.cpu().numpy()
            stats.append(st.cpu().numpy())
            for i, t in kept.items():
                parts[i].append(t.cpu().numpy())
        self._handle_debug_output(ids, np.concatenate(stats, axis=1), parts)
        return out

    def _handle_debug_output(self, ids, stats, parts):
        """base.py:769-802 from the per-row statistics (n_tensors, N, 4) and the kept chunks: the reference reduces each tensor
        over the whole batch."""
        mn = [np.float32(np.min(stats[k, :, 0])) for k in range(len(ids))]           # (np.min / np.max: NaN where a row's is NaN)
        mx = [np.float32(np.max(stats[k, :, 1])) for k in range(len(ids))]
        nonfinite = [int(stats[k, :, 3].sum()) for k in range(len(ids))]
        self._reversed_stats = dict((i, {"min": float(mn[k]), "max": float(mx[k]), "sum": stats[k, :, 2].copy(), "nonfinite": nonfinite[k]})
                                    for k, i in enumerate(ids))
        if self._reverse_check_min_max_values:
            print("Minimum values in tensors: "
                  "((NodeID, TensorID), Value) - {}".format(sorted(zip(ids, mn), key=lambda t: t[0])))
            print("Maximum values in tensors: "
                  "((NodeID, TensorID), Value) - {}".format(sorted(zip(ids, mx), key=lambda t: t[0])))
        if self._reverse_check_finite:
            bad = sorted(i for k, i in enumerate(ids) if nonfinite[k] > 0)
            if bad:
                print("Not finite values found in following nodes: "
                      "(NodeID, TensorID) - {}".format(bad))
        if self._reverse_keep_tensors:
            self._reversed_tensors = sorted(((i, np.concatenate(parts[i], axis=0)) for i in ids), key=lambda t: t[0])


def infer_alpha_beta(alpha, beta, caller):
    """(alpha, beta) of an alpha-beta rule under the reference's conditions (relevance_based/utils.py:72-129): alpha >= 1,
    beta >= 0, alpha - beta == 1; either one may be None and follows from the other.  `caller`: the class name the reference
    puts in front of its message.  The messages are the reference's."""
    head = "Constructor call to {} : ".format(caller)
    if alpha is None and beta is None:
        raise ValueError(head + "Neither alpha or beta were given")
    if alpha is not None and alpha < 1:
        raise ValueError(head + "Passed parameter alpha invalid. Expecting alpha >= 1 but was {}".format(alpha))
    if beta is not None and beta < 0:
        raise ValueError(head + "Passed parameter beta invalid. Expecting beta >= 0 but was {}".format(beta))
    if alpha is None:
        alpha = beta + 1
        if alpha < 1:
            raise ValueError(head + "Inferring alpha from given beta {} s.t. alpha - beta = 1, with condition alpha >= 1 not possible.".format(beta))
    if beta is None:
        beta = alpha - 1
        if beta < 0:
            raise ValueError(head + "Inferring beta from given alpha {} s.t. alpha - beta = 1, with condition beta >= 0 not possible.".format(alpha))
    if alpha - beta != 1:
        raise ValueError(head + "Condition alpha - beta = 1 not fulfilled. alpha={} ; beta={} -> alpha - beta = {}".format(alpha, beta, alpha - beta))
    return alpha, beta


class LRPAlphaBeta(LRPSequentialPresetA):
    """relevance_analyzer.py:578-620: every conv under AlphaBetaRule(alpha, beta, bias=True) (relevance_rule.py:216-322), max-pools
    by gradient routing — the same `analyze([X, R])` surface as LRPSequentialPresetA, on the engine's walk under
    lrp_set_cnn_rule(alpha, beta).  (1, 0) is LRPSequentialPresetA's walk to the bit; beta > 0 runs the two-chain walk
    (VGG-style encoders, and a ResNet `ImageModelSpec` whose widths are multiples of 8).  bias=False is refused here: the IgnoreBias rules run on the rule table (LRPAlpha2Beta1IgnoreBias,
    LRPAlpha1Beta0IgnoreBias, or LRP(model, rule=("alphabeta", alpha, beta, False)))."""

    def __init__(self, model, alpha=None, beta=None, bias=True, neuron_selection_mode="replace", **kwargs):
        alpha, beta = infer_alpha_beta(alpha, beta, self.__class__.__name__)
        if not bias:
            raise NotImplementedError("bias=False: use LRPAlpha2Beta1IgnoreBias / LRPAlpha1Beta0IgnoreBias or LRP(model, rule=('alphabeta', alpha, beta, False))")
        self._alpha, self._beta, self._bias = alpha, beta, bias
        super(LRPAlphaBeta, self).__init__(model, neuron_selection_mode=neuron_selection_mode, **kwargs)
        self._engine.set_cnn_rule(alpha, beta)


class LRPAlpha2Beta1(LRPAlphaBeta):
    """relevance_analyzer.py:635-642."""

    def __init__(self, model, **kwargs):
        super(LRPAlpha2Beta1, self).__init__(model, alpha=2, beta=1, bias=True, **kwargs)


class LRPAlpha1Beta0(LRPAlphaBeta):
    """relevance_analyzer.py:655-662."""

    def __init__(self, model, **kwargs):
        super(LRPAlpha1Beta0, self).__init__(model, alpha=1, beta=0, bias=True, **kwargs)


class LRPSequentialPresetB(LRPAlphaBeta):
    """relevance_analyzer.py:724-748: Dense -> EpsilonRule(epsilon), Conv -> Alpha2Beta1Rule.  The truncated encoders have no
    Dense layer, so epsilon is validated and stored as LRPSequentialPresetA does."""

    def __init__(self, model, epsilon=0.1, **kwargs):
        super(LRPSequentialPresetB, self).__init__(model, alpha=2, beta=1, bias=True, epsilon=epsilon, **kwargs)


# ---------------------------------------------------------------------------------------------------------------------
# Rule table: LRP(model, rule=..., input_layer_rule=...) (relevance_analyzer.py:300-415) on lrp_set_cnn_rules
# ---------------------------------------------------------------------------------------------------------------------
class _Rule(object):
    """A conv rule of relevance_rule.py as data: subclass and override the class attributes to pass parameters, as the
    reference's proxy classes do (relevance_analyzer.py:538-548)."""
    _kind = None
    alpha, beta, bias, epsilon, low, high = None, None, True, 1e-7, -1, 1

    @classmethod
    def spec(cls):
        if cls._kind == "alphabeta":
            a, b = infer_alpha_beta(cls.alpha, cls.beta, cls.__name__)
            return ("alphabeta", a, b, bool(cls.bias))
        if cls._kind == "epsilon":
            return ("epsilon", check_epsilon(cls.epsilon, cls.__name__), bool(cls.bias))
        if cls._kind == "z":
            return ("epsilon", 0.0, bool(cls.bias))
        if cls._kind == "bounded":
            return ("bounded", cls.low, cls.high)
        if cls._kind in ("flat", "wsquare"):
            return (cls._kind,)
        raise NotImplementedError("%s: %s" % (cls.__name__, cls.__doc__))


def check_epsilon(epsilon, caller):
    """relevance_based/utils.py:52-69."""
    if epsilon <= 0:
        raise ValueError("Constructor call to {} : Parameter epsilon must be > 0 but was {}".format(caller, epsilon))
    return epsilon


class ZRule(_Rule): _kind = "z"                                                         # RR:74-98
class ZIgnoreBiasRule(ZRule): bias = False                                              # RR:102-109
class EpsilonRule(_Rule): _kind = "epsilon"                                             # RR:113-144
class EpsilonIgnoreBiasRule(EpsilonRule): bias = False                                  # RR:148-152
class WSquareRule(_Rule): _kind = "wsquare"                                             # RR:156-187
class FlatRule(_Rule): _kind = "flat"                                                   # RR:192-211
class AlphaBetaRule(_Rule): _kind = "alphabeta"                                         # RR:216-322
class AlphaBetaIgnoreBiasRule(AlphaBetaRule): bias = False                              # RR:327-331
class Alpha2Beta1Rule(AlphaBetaRule): alpha, beta = 2, 1                                # RR:335-341
class Alpha2Beta1IgnoreBiasRule(Alpha2Beta1Rule): bias = False                          # RR:344-350
class Alpha1Beta0Rule(AlphaBetaRule): alpha, beta = 1, 0                                # RR:353-359
class Alpha1Beta0IgnoreBiasRule(Alpha1Beta0Rule): bias = False                          # RR:362-368
class BoundedRule(_Rule): _kind = "bounded"                                             # RR:372-441
class ZPlusRule(Alpha1Beta0IgnoreBiasRule): pass                                        # RR:445-456


class ZPlusFastRule(_Rule):
    """not built: its one-conv form assumes x >= 0, which the image layer's mean-subtracted input is not; use ZPlus"""


LRP_RULES = {"Z": ZRule, "ZIgnoreBias": ZIgnoreBiasRule, "Epsilon": EpsilonRule, "EpsilonIgnoreBias": EpsilonIgnoreBiasRule,
             "WSquare": WSquareRule, "Flat": FlatRule, "AlphaBeta": AlphaBetaRule, "AlphaBetaIgnoreBias": AlphaBetaIgnoreBiasRule,
             "Alpha2Beta1": Alpha2Beta1Rule, "Alpha2Beta1IgnoreBias": Alpha2Beta1IgnoreBiasRule, "Alpha1Beta0": Alpha1Beta0Rule,
             "Alpha1Beta0IgnoreBias": Alpha1Beta0IgnoreBiasRule, "ZPlus": ZPlusRule, "ZPlusFast": ZPlusFastRule,
             "Bounded": BoundedRule}                                                     # relevance_analyzer.py:173-194

_INPUT_ONLY = ("flat", "wsquare", "bounded")


def normalize_rule(rule):
    """One conv's rule -> the record LRPEngine.set_cnn_rules takes: a name of LRP_RULES, one of the rule classes above, or the
    record itself — ("alphabeta", alpha, beta, bias), ("epsilon", eps, bias) with eps = 0 for ZRule, ("flat",), ("wsquare",),
    ("bounded", low, high)."""
    if isinstance(rule, str):
        if rule not in LRP_RULES:
            raise ValueError("unknown LRP rule %r: one of %s" % (rule, sorted(LRP_RULES)))
        rule = LRP_RULES[rule]
    if isinstance(rule, type) and issubclass(rule, _Rule):
        return rule.spec()
    if not isinstance(rule, (tuple, list)) or not rule or not isinstance(rule[0], str):
        raise ValueError("not an LRP rule: %r" % (rule,))
    kind, args = rule[0], tuple(rule[1:])
    if kind == "alphabeta" and len(args) in (2, 3):
        a, b = infer_alpha_beta(args[0], args[1], "AlphaBetaRule")
        return ("alphabeta", a, b, bool(args[2]) if len(args) == 3 else True)
    if kind == "epsilon" and len(args) in (1, 2):
        if not args[0] >= 0:
            raise ValueError("epsilon must be >= 0 but was {}".format(args[0]))
        return ("epsilon", float(args[0]), bool(args[1]) if len(args) == 2 else True)
    if kind == "bounded" and len(args) == 2:
        if not args[0] < args[1]:
            raise ValueError("BoundedRule needs low < high but got ({}, {})".format(*args))
        return ("bounded", float(args[0]), float(args[1]))
    if kind in ("flat", "wsquare") and not args:
        return (kind,)
    raise ValueError("not an LRP rule: %r" % (rule,))


def rule_table(rule, input_layer_rule, n_conv):
    """The per-conv table of LRP(model, rule=..., input_layer_rule=...), input layer first (relevance_analyzer.py:343-415).
    rule: one rule for every conv, or a list with one per conv in the reference's order — create_rule_mapping pops from the END
    while the graph is walked in reverse, so the list reads input layer first, and with an input_layer_rule (inserted at index
    0, RA:395) it holds the convs above the image layer only.  input_layer_rule: a rule, or (low, high) for BoundedRule."""
    if rule is None:
        raise ValueError("Need LRP rule(s).")                                              # RA:345-346
    if input_layer_rule is not None:
        if isinstance(input_layer_rule, tuple) and len(input_layer_rule) == 2 and not isinstance(input_layer_rule[0], str):
            input_layer_rule = ("bounded",) + tuple(input_layer_rule)                      # RA:379-386
        input_layer_rule = normalize_rule(input_layer_rule)
    if isinstance(rule, list):
        if rule and isinstance(rule[0], tuple) and len(rule[0]) == 2 and callable(rule[0][0]):
            raise NotImplementedError("conditional rule lists need the Keras graph; give one rule per conv")
        table = [normalize_rule(r) for r in rule]
        if input_layer_rule is not None:
            table.insert(0, input_layer_rule)
        if len(table) != n_conv:
            raise ValueError("%d rules for %d layers with a kernel" % (len(table), n_conv))
    else:
        table = [normalize_rule(rule)] * n_conv
        if input_layer_rule is not None:
            table[0] = input_layer_rule
    for i, r in enumerate(table):
        if r[0] in _INPUT_ONLY and i > 0:
            raise NotImplementedError("%s above the input layer is not built: it sends relevance to units whose ReLU is off, "
                                      "which the cached gates a / Z cannot carry" % r[0])
    return tuple(table)


def resnet_rule_pair(rule, input_layer_rule=None):
    """The rule pair of a ResNet encoder (LRPEngine.set_resnet_rules) from the keywords of LRP(...): -> (stem record, record of
    every other conv).  rule: ONE rule; a list is refused — the reference pops list entries in its graph-reversal order of the
    branched graph, which is not reproduced.  input_layer_rule: a rule, or (low, high) for BoundedRule; None: `rule` at the stem too."""
    if rule is None:
        raise ValueError("Need LRP rule(s).")                                              # RA:345-346
    if isinstance(rule, list):
        raise NotImplementedError("a list with a rule per conv on a ResNet encoder: the reference's list order over the branched graph "
                                  "is not reproduced; give one rule and an input_layer_rule")
    units = normalize_rule(rule)
    if units[0] in _INPUT_ONLY:
        raise NotImplementedError("%s above the input layer is not built: it sends relevance to units whose ReLU is off, "
                                  "which the cached gates cannot carry" % units[0])
    if input_layer_rule is None:
        return units, units
    if isinstance(input_layer_rule, tuple) and len(input_layer_rule) == 2 and not isinstance(input_layer_rule[0], str):
        input_layer_rule = ("bounded",) + tuple(input_layer_rule)                          # RA:379-386
    return normalize_rule(input_layer_rule), units


class LRP(LRPSequentialPresetA):
    """relevance_analyzer.py:300-500 for the truncated encoders: `rule` for every conv (a name of LRP_RULES, a rule class, a record
    of normalize_rule, or — VGG-style encoders — a list per conv), `input_layer_rule` for the image layer (a rule, or (low, high)
    for BoundedRule); pools by gradient routing.  Same analyze([X, R]) surface; the engine runs the table walk of
    lrp_set_cnn_rules, on a ResNet `ImageModelSpec` the rule pair of lrp_set_resnet_rules (BatchNorm, Add and the pad reversed as
    under every other analyzer).  Epsilon and Z rules switch the engine to exact fp32, as the gradient analyzers do.

    One deviation on a ResNet encoder: the reference selects the input rule by `is_input_layer` (checks.py:394-424), which is
    false for Keras ResNet's `conv1_conv` because `conv1_pad` sits in front of it, so with a single rule it silently never
    applies `input_layer_rule` on this model.  Here the input rule applies at the stem conv: what the caller asks for, and what
    the reference's list form does.  A `rule=[...]` list on a ResNet spec stays NotImplementedError."""

    def __init__(self, model, rule=None, input_layer_rule=None, neuron_selection_mode="replace", **kwargs):
        if rule is None:
            raise ValueError("Need LRP rule(s).")                                          # RA:345-346
        resnet = getattr(model, "resnet", None) is not None
        table = resnet_rule_pair(rule, input_layer_rule) if resnet else rule_table(rule, input_layer_rule, len(model.cnn_cfg))
        self._rule, self._input_layer_rule, self._table = rule, input_layer_rule, table
        super(LRP, self).__init__(model, neuron_selection_mode=neuron_selection_mode, **kwargs)
        if any(r[0] == "epsilon" for r in table):
            self._engine.set_precision("fp32")
        if resnet:
            self._engine.set_resnet_rules(table[1], table[0])
        else:
            self._engine.set_cnn_rules(table)


class LRPZ(LRP):
    """relevance_analyzer.py:517-520."""

    def __init__(self, model, **kwargs):
        super(LRPZ, self).__init__(model, rule="Z", **kwargs)


class LRPZIgnoreBias(LRP):
    """relevance_analyzer.py:523-527."""

    def __init__(self, model, **kwargs):
        super(LRPZIgnoreBias, self).__init__(model, rule="ZIgnoreBias", **kwargs)


class LRPEpsilon(LRP):
    """relevance_analyzer.py:531-552."""

    def __init__(self, model, epsilon=1e-7, bias=True, **kwargs):
        self._epsilon_rule = check_epsilon(epsilon, self.__class__.__name__)
        super(LRPEpsilon, self).__init__(model, rule=("epsilon", epsilon, bias), **kwargs)


class LRPEpsilonIgnoreBias(LRPEpsilon):
    """relevance_analyzer.py:555-561."""

    def __init__(self, model, epsilon=1e-7, **kwargs):
        super(LRPEpsilonIgnoreBias, self).__init__(model, epsilon=epsilon, bias=False, **kwargs)


class LRPAlpha2Beta1IgnoreBias(LRP):
    """relevance_analyzer.py:649-656."""

    def __init__(self, model, **kwargs):
        super(LRPAlpha2Beta1IgnoreBias, self).__init__(model, rule="Alpha2Beta1IgnoreBias", **kwargs)


class LRPAlpha1Beta0IgnoreBias(LRP):
    """relevance_analyzer.py:669-676."""

    def __init__(self, model, **kwargs):
        super(LRPAlpha1Beta0IgnoreBias, self).__init__(model, rule="Alpha1Beta0IgnoreBias", **kwargs)


class LRPZPlus(LRPAlpha1Beta0IgnoreBias):
    """relevance_analyzer.py:678-681."""


class LRPSequentialPresetAFlat(LRP):
    """relevance_analyzer.py:755-760: LRPSequentialPresetA with FlatRule at the image layer."""

    def __init__(self, model, epsilon=0.1, **kwargs):
        super(LRPSequentialPresetAFlat, self).__init__(model, rule="Alpha1Beta0", input_layer_rule=FlatRule, epsilon=epsilon, **kwargs)


class LRPSequentialPresetBFlat(LRP):
    """relevance_analyzer.py:765-770: LRPSequentialPresetB with FlatRule at the image layer."""

    def __init__(self, model, epsilon=0.1, **kwargs):
        super(LRPSequentialPresetBFlat, self).__init__(model, rule="Alpha2Beta1", input_layer_rule="Flat", epsilon=epsilon, **kwargs)


class _NotBuilt(object):
    _why = ""

    def __init__(self, model=None, *args, **kwargs):
        raise NotImplementedError("%s: %s" % (self.__class__.__name__, self._why))


class LRPFlat(_NotBuilt):
    """relevance_analyzer.py:571-575."""
    _why = "FlatRule above the input layer needs relevance at units whose ReLU is off; use input_layer_rule='Flat'"


class LRPWSquare(_NotBuilt):
    """relevance_analyzer.py:564-568."""
    _why = "WSquareRule above the input layer needs relevance at units whose ReLU is off; use input_layer_rule='WSquare'"


class LRPZPlusFast(_NotBuilt):
    """relevance_analyzer.py:684-692."""
    _why = "its one-conv form assumes x >= 0, which the mean-subtracted image is not; LRPZPlus is the same rule without that assumption"


class BaselineLRPZ(_NotBuilt):
    """relevance_analyzer.py:57-100."""
    _why = "input x gradient of the whole model; InputTimesGradient is that walk, and LRPZ the rule-based one"


PRESETS = {  # CaptionModelSpec(cnn_rule=<name>): (rule, input_layer_rule)
    "presetA": ("Alpha1Beta0", None), "presetB": ("Alpha2Beta1", None), "presetAflat": ("Alpha1Beta0", "Flat"),
    "presetBflat": ("Alpha2Beta1", "Flat"), "alpha2beta1ignorebias": ("Alpha2Beta1IgnoreBias", None),
    "alpha1beta0ignorebias": ("Alpha1Beta0IgnoreBias", None), "zplus": ("ZPlus", None), "z": ("Z", None),
    "zignorebias": ("ZIgnoreBias", None)}


def _check_selection_mode(neuron_selection_mode):
    if neuron_selection_mode not in ["max_activation", "index", "all", "replace"]:
        raise ValueError("neuron_selection parameter is not valid.")             # base.py:332-333
    if neuron_selection_mode != "replace":
        raise NotImplementedError("only neuron_selection_mode='replace' is on the captioning hot path")


class _GradientWalkAnalyzer(object):
    """`analyze([X, head])` of a gradient_based analyzer on the engine's encoder walk (lrp_cnn_walk)."""
    _walk = "gradient"

    def __init__(self, model, neuron_selection_mode="replace", max_batch=8, device=None):
        _check_selection_mode(neuron_selection_mode)
        self._neuron_selection_mode = neuron_selection_mode
        self._model = model
        h, w, c = model.output_shape()
        self._engine = LRPEngine(decoder="adaptive", cnn_cfg=model.cnn_cfg, img_hw=model.img_hw, L=h * w, D=c, H=8, E=8,
                                 V=4, max_images=max_batch, max_tokens=max_batch, max_caption_len=2, device=device,
                                 resnet=model.resnet)
        self._engine.set_weights(model.weights)
        self._engine.set_precision("fp32")

    def _walk_of_call(self):
        return self._walk

    def _finish(self, g, img):
        return g

    def analyze(self, X, neuron_selection=None):
        if neuron_selection is not None:
            raise ValueError("Only neuron_selection_mode 'index' expects the neuron_selection parameter.")  # base.py:489-492
        X = list(X) if isinstance(X, (list, tuple)) else [X]
        if len(X) != 2:
            raise ValueError("neuron_selection_mode 'replace' expects [X, head]")
        img, R = np.asarray(X[0], dtype=np.float32), np.asarray(X[1], dtype=np.float32)
        n = img.shape[0]
        if R.shape[0] != n:
            raise ValueError("X and head must have the same batch size")
        e = self._engine
        out = np.empty_like(img)
        for lo in range(0, n, e.max_images):
            hi = min(n, lo + e.max_images, lo + e.max_tokens)
            e.encode_images(img[lo:hi])
            g = e.cnn_walk(list(range(hi - lo)), R[lo:hi].reshape(hi - lo, e.L, e.D), self._walk_of_call()).cpu().numpy()
            out[lo:hi] = self._finish(g, img[lo:hi])
        return out


class Gradient(_GradientWalkAnalyzer):
    """gradient_based.py:101-151: the gradient of the head-weighted output w.r.t. the input, optionally |.| or squared."""

    def __init__(self, model, postprocess=None, **kwargs):
        if postprocess not in [None, "abs", "square"]:
            raise ValueError("Parameter 'postprocess' must be either None, 'abs', or 'square'.")   # :110-112
        self._postprocess = postprocess
        super(Gradient, self).__init__(model, **kwargs)

    def _post(self, g):
        if self._postprocess == "abs":
            return np.abs(g)
        if self._postprocess == "square":
            return np.square(g)
        return g

    def _finish(self, g, img):
        return self._post(g)


class InputTimesGradient(Gradient):
    """gradient_based.py:154-176: X times the (post-processed) gradient.  Without a post-processing step the product is taken
    on the device (the walk's Input x Gradient stem); with one, the gradient is post-processed first, as in the reference."""
    _walk = "input_x_gradient"

    def _walk_of_call(self):
        return "input_x_gradient" if self._postprocess is None else "gradient"

    def _finish(self, g, img):
        return g if self._postprocess is None else img * self._post(g)


class GuidedBackprop(_GradientWalkAnalyzer):
    """gradient_based.py:228-265: every layer with a ReLU first clamps the arriving value at 0, then applies its gradient."""
    _walk = "guided_backprop"


class Deconvnet(_GradientWalkAnalyzer):
    """gradient_based.py:180-225: every layer with a ReLU clamps the arriving value at 0 and applies the gradient of the layer
    WITHOUT its activation — no forward ReLU decision is read; max-pools route to the forward's arg-max."""
    _walk = "deconvnet"


def check_deeplift_reference(reference_inputs, img_hw):
    """reference_inputs of DeepLIFT as the engine takes it: a finite scalar, or an array that broadcasts to (1, H, W, 3) — one
    reference for all images (utils/keras/__init__.py:60-74)."""
    if isinstance(reference_inputs, (str, bytes)) or reference_inputs is None:
        raise ValueError("reference_inputs must be a number or an array")
    ref = np.asarray(reference_inputs, dtype=np.float32)
    if not np.all(np.isfinite(ref)):
        raise ValueError("reference_inputs must be finite")
    if ref.ndim:
        try:
            np.broadcast_to(ref, (1, img_hw[0], img_hw[1], 3))
        except ValueError:
            raise ValueError("reference_inputs of shape %s does not broadcast to (1, %d, %d, 3): one reference is shared by all "
                             "images" % (ref.shape, img_hw[0], img_hw[1]))
    return ref


class DeepLIFT(_GradientWalkAnalyzer):
    """deeplift.py:44-250 for the VGG-style encoders, `analyze([X, head])`: LinearRule on every fused conv + ReLU layer against
    the forward of `reference_inputs` (a scalar or an array that broadcasts to (1, H, W, 3)), the pools by gradient routing;
    approximate_gradient as in the reference (the gradient where |x - reference| < 1e-7).  Runs on the engine's DeepLIFT walk
    (lrp_set_deeplift_reference, LRP_WALK_DEEPLIFT) in exact fp32.  A ResNet spec is NotImplementedError: its stand-alone
    Activation, BatchNorm and Add layers take other mappings, and that walk is not built."""
    _walk = "deeplift"

    def __init__(self, model, reference_inputs=0, approximate_gradient=True, neuron_selection_mode="replace", max_batch=8,
                 device=None):
        _check_selection_mode(neuron_selection_mode)
        if getattr(model, "resnet", None) is not None:
            raise NotImplementedError("DeepLIFT is built for the VGG-style (conv-list) encoders only")
        ref = check_deeplift_reference(reference_inputs, model.img_hw)
        self._reference_inputs, self._approximate_gradient = ref, bool(approximate_gradient)
        super(DeepLIFT, self).__init__(model, neuron_selection_mode=neuron_selection_mode, max_batch=max_batch, device=device)
        self._engine.set_deeplift_reference(ref, self._approximate_gradient)


class DeepLIFTWrapper(object):
    """deeplift.py:253-: the wrapper around the `deeplift` package, which the reference imports in its constructor."""

    def __init__(self, model=None, *args, **kwargs):
        raise ImportError("To use DeepLIFTWrapper please install the python module 'deeplift', "
                          "e.g.: 'pip install deeplift'")


class PatternNet(_GradientWalkAnalyzer):
    """pattern_based.py:128-247 for the VGG-style encoders, `analyze([X, head])` on the engine's 'patternnet' walk
    (LRP_WALK_PATTERNNET, exact fp32): per conv + ReLU layer the ReLU's gradient, then the conv's gradient with the kernel replaced
    by the layer's pattern; reverse_project_bottleneck_layers (default True) divides every reversed tensor by its absolute maximum.
    patterns: one (3, 3, cin, cout) array per conv, e.g. from pattern.PatternComputer; None: call fit / fit_generator first
    (pattern_type, default 'relu').  The other reverse_* switches are not built for this walk.  A ResNet spec is refused as the
    reference refuses BatchNorm and Add layers."""
    _walk = "patternnet"
    _REVERSE_SWITCHES = ("reverse_keep_tensors", "reverse_check_min_max_values", "reverse_check_finite", "reverse_clip_values",
                         "reverse_verbose")

    def __init__(self, model, patterns=None, pattern_type=None, **kwargs):
        if getattr(model, "resnet", None) is not None:
            raise NotAnalyzeableModelException("PatternNet is only well defined for conv2d/max-pooling/dense layers.")   # :161-166
        for k in self._REVERSE_SWITCHES:
            if kwargs.pop(k, False):
                raise NotImplementedError("%s is not built for the pattern walks" % k)
        self._project = bool(kwargs.pop("reverse_project_bottleneck_layers", True))
        if not self._project:
            import warnings
            warnings.warn("The standard setting for 'reverse_project_bottleneck_layers' is overwritten.")       # :178-181
        self._patterns = list(patterns) if patterns is not None else None
        self._pattern_type = pattern_type
        super(PatternNet, self).__init__(model, **kwargs)
        self._engine.set_pattern_projection(self._project)
        if self._patterns is not None:
            self._engine.set_patterns(self._patterns)

    def fit(self, X=None, batch_size=32, **kwargs):
        """base.py:248-257: the patterns from the data X (N, H, W, 3), batch_size images at a time."""
        X = np.asarray(X, dtype=np.float32)
        return self.fit_generator(X[lo:lo + batch_size] for lo in range(0, len(X), batch_size))

    def fit_generator(self, generator, **kwargs):
        """pattern_based.py:209-243: one pass over the batches the generator yields (arrays, or [array] lists)."""
        pattern_type = "relu" if self._pattern_type is None else self._pattern_type
        if isinstance(pattern_type, (list, tuple)):
            raise ValueError("Only one pattern type allowed. Please pass a string.")                                # :228-230
        from .pattern import fit_engine
        self._patterns = fit_engine(self._engine, generator, pattern_type)

    def analyze(self, X, neuron_selection=None):
        if self._patterns is None:
            raise RuntimeError("no patterns: pass patterns= or call fit / fit_generator before analyze")
        return super(PatternNet, self).analyze(X, neuron_selection=neuron_selection)


class PatternAttribution(PatternNet):
    """pattern_based.py:250-281: PatternNet with the kernel replaced by pattern * kernel ('pattern_attribution' walk)."""
    _walk = "pattern_attribution"


class DeepTaylor(LRP):
    """deeptaylor.py:40-160 for the VGG-style encoders: Alpha1Beta0Rule (with the bias) on every fused conv, the pools by gradient
    routing, and a ReLU on the output — whose mask is already in the top layer's gate (a = 0 there gives G = 0).  That is the
    engine's default walk.  A ResNet spec is NotImplementedError (its BatchNorm layers are `do_nothing` there, another walk)."""

    def __init__(self, model, neuron_selection_mode="replace", **kwargs):
        if getattr(model, "resnet", None) is not None:
            raise NotImplementedError("DeepTaylor is built for the VGG-style (conv-list) encoders only")
        super(DeepTaylor, self).__init__(model, rule="Alpha1Beta0", input_layer_rule=self._input_rule(),
                                         neuron_selection_mode=neuron_selection_mode, **kwargs)

    def _input_rule(self):
        return None

    def analyze(self, X, neuron_selection=None):
        """The head passes the output ReLU's gradient mapping first (deeptaylor.py:69-75, :144-154): head [feat > 0].  The top
        layer's rule divides by Z+ and has no gate of its own, so this mask is the one thing the default walk does not hold."""
        if neuron_selection is not None:
            raise ValueError("Only neuron_selection_mode 'index' expects the neuron_selection parameter.")  # base.py:489-492
        if self._trace:
            return self._analyze_traced(X, mask_head=True)
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
            head = R[lo:hi].reshape(hi - lo, e.L, e.D) * (e.get_features()[:hi - lo].cpu().numpy() > 0)
            out[lo:hi] = e.cnn_explain(list(range(hi - lo)), head).cpu().numpy()
        return out


class BoundedDeepTaylor(DeepTaylor):
    """deeptaylor.py:163-199: DeepTaylor with BoundedRule(low, high) at the image layer."""

    def __init__(self, model, low=None, high=None, **kwargs):
        if low is None or high is None:
            raise ValueError("The low or high parameter is missing. Z-B (bounded rule) require both values.")   # :172-175
        if not (float(low) < float(high)):
            raise ValueError("bounded rule: low < high (low=%r, high=%r)" % (low, high))
        self._bounds = (float(low), float(high))
        super(BoundedDeepTaylor, self).__init__(model, **kwargs)

    def _input_rule(self):
        return self._bounds


# ---------------------------------------------------------------------------------------------------------------------
# AugmentReduceBase wrappers (wrapper.py:78-345) on LRPEngine.cnn_walk_augmented
# ---------------------------------------------------------------------------------------------------------------------
def _engine_walk(subanalyzer):
    """(walk, postprocess) of an analyzer of this module that runs on an engine walk: the four gradient-walk classes and the
    LRP classes (the 'lrp' walk under the subanalyzer's own rule and precision)."""
    if isinstance(subanalyzer, DeepLIFT):
        raise TypeError("DeepLIFT is not built under an augmenting wrapper")
    if isinstance(subanalyzer, _GradientWalkAnalyzer):
        post = getattr(subanalyzer, "_postprocess", None)
        if isinstance(subanalyzer, InputTimesGradient) and post is not None:
            raise NotImplementedError("InputTimesGradient with a postprocess under a wrapper: the product with the sample "
                                      "follows the post-processing; wrap Gradient(postprocess=...) instead")
        return subanalyzer._walk, post
    if isinstance(subanalyzer, LRPSequentialPresetA):
        return "lrp", None
    raise TypeError("the wrappers take an analyzer of this module that runs on an engine walk (Gradient, InputTimesGradient, "
                    "GuidedBackprop, Deconvnet or an LRP class), not %r" % (type(subanalyzer).__name__,))


class AugmentReduceBase(object):
    """wrapper.py:78-206 with `analyze([X, head])`: every input is augmented to augment_by_n samples, each sample explained by the
    subanalyzer's engine walk, and the maps reduced to their mean — all on the device (LRPEngine.cnn_walk_augmented); only the
    (N, H, W, 3) result comes back.  One deviation from the reference: its wrappers silently switch the subanalyzer to
    neuron_selection_mode 'index' (wrapper.py:84-86) and so cannot run with a replaced head at all; here the mode stays
    'replace' and the head stays the caller's, repeated for each of its image's samples."""
    _kind = None

    @staticmethod
    def _check_n(augment_by_n):
        if isinstance(augment_by_n, bool) or int(augment_by_n) != augment_by_n or augment_by_n < 1:
            raise ValueError("augment_by_n must be a positive integer but was {}".format(augment_by_n))

    def __init__(self, subanalyzer, augment_by_n=2, max_batch=None):
        self._check_n(augment_by_n)
        self._walk, self._post = _engine_walk(subanalyzer)
        self._augment_by_n = int(augment_by_n)
        self._subanalyzer = subanalyzer
        self._neuron_selection_mode = subanalyzer._neuron_selection_mode
        self._max_batch = max_batch

    def _augment_args(self):
        return {}

    def analyze(self, X, neuron_selection=None):
        if neuron_selection is not None:
            raise ValueError("Only neuron_selection_mode 'index' expects the neuron_selection parameter.")  # base.py:489-492
        X = list(X) if isinstance(X, (list, tuple)) else [X]
        if len(X) != 2:
            raise ValueError("neuron_selection_mode 'replace' expects [X, head]")
        img, R = np.asarray(X[0], dtype=np.float32), np.asarray(X[1], dtype=np.float32)
        if R.shape[0] != img.shape[0]:
            raise ValueError("X and head must have the same batch size")
        e = self._subanalyzer._engine
        out = e.cnn_walk_augmented(img, R.reshape(img.shape[0], e.L, e.D), self._walk, self._kind, self._augment_by_n,
                                   postprocess=self._post, max_batch=self._max_batch, **self._augment_args())
        return out.cpu().numpy()


class GaussianSmoother(AugmentReduceBase):
    """wrapper.py:214-242: sample = x + N(0, noise_scale).  The draw is the device generator of lrp_op_augment_gaussian
    (Philox4x32-10 + Box-Muller, a pure function of (seed, sample row, element)), not numpy's / TensorFlow's."""
    _kind = "gaussian"

    @staticmethod
    def _check_noise(noise_scale, seed):
        if not noise_scale >= 0:
            raise ValueError("noise_scale must be >= 0 but was {}".format(noise_scale))
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be an integer in [0, 2^64)")

    def __init__(self, subanalyzer, augment_by_n=2, noise_scale=1, seed=0, **kwargs):
        self._check_noise(noise_scale, seed)
        super(GaussianSmoother, self).__init__(subanalyzer, augment_by_n=augment_by_n, **kwargs)
        self._noise_scale, self._seed = float(noise_scale), int(seed)

    def _augment_args(self):
        return {"noise_scale": self._noise_scale, "seed": self._seed}


class PathIntegrator(AugmentReduceBase):
    """wrapper.py:250-345: the mean of the subanalyzer's maps over `steps` points of a path, times (x - reference_inputs).
    path='reference' is literally what the reference computes — x + (s / steps) (x - reference), s = 0 .. steps - 1: it starts
    at x and moves AWAY from the reference (wrapper.py:268-288, :317-337) — and path='standard' the published straight path
    reference + (s / steps) (x - reference).  reference_inputs: a scalar, or an array that broadcasts to X."""
    _kind = "path"

    @staticmethod
    def _check_path(reference_inputs, path):
        if path not in ("reference", "standard"):
            raise ValueError("path must be 'reference' or 'standard'")
        if isinstance(reference_inputs, (str, bytes)):
            raise ValueError("reference_inputs must be a number or an array")
        return reference_inputs if np.isscalar(reference_inputs) else np.asarray(reference_inputs, dtype=np.float32)

    def __init__(self, subanalyzer, steps=16, reference_inputs=0, path="reference", **kwargs):
        reference_inputs = self._check_path(reference_inputs, path)
        super(PathIntegrator, self).__init__(subanalyzer, augment_by_n=steps, **kwargs)
        self._reference_inputs, self._path = reference_inputs, path

    def _augment_args(self):
        return {"reference": self._reference_inputs, "path": self._path}


def _check_wrapped_gradient(postprocess, neuron_selection_mode):
    """what Gradient(model, ...) refuses, asked before the wrapper's own checks so that nothing is created on a bad argument"""
    _check_selection_mode(neuron_selection_mode)
    if postprocess not in [None, "abs", "square"]:
        raise ValueError("Parameter 'postprocess' must be either None, 'abs', or 'square'.")   # gradient_based.py:110-112


class SmoothGrad(GaussianSmoother):
    """gradient_based.py:300-319: GaussianSmoother over Gradient(model, postprocess)."""

    def __init__(self, model, augment_by_n=64, postprocess=None, neuron_selection_mode="replace", noise_scale=1, seed=0,
                 max_batch=8, device=None):
        _check_wrapped_gradient(postprocess, neuron_selection_mode)
        self._check_n(augment_by_n)
        self._check_noise(noise_scale, seed)
        sub = Gradient(model, postprocess=postprocess, neuron_selection_mode=neuron_selection_mode, max_batch=max_batch, device=device)
        super(SmoothGrad, self).__init__(sub, augment_by_n=augment_by_n, noise_scale=noise_scale, seed=seed)


class IntegratedGradients(PathIntegrator):
    """gradient_based.py:273-292: PathIntegrator over Gradient(model, postprocess)."""

    def __init__(self, model, steps=64, postprocess=None, neuron_selection_mode="replace", reference_inputs=0, path="reference",
                 max_batch=8, device=None):
        _check_wrapped_gradient(postprocess, neuron_selection_mode)
        self._check_n(steps)
        self._check_path(reference_inputs, path)
        sub = Gradient(model, postprocess=postprocess, neuron_selection_mode=neuron_selection_mode, max_batch=max_batch, device=device)
        super(IntegratedGradients, self).__init__(sub, steps=steps, reference_inputs=reference_inputs, path=path)


# innvestigate/analyzer/__init__.py:35-85, the entries this module builds under the reference's keys (pattern.*,
# gradient.baseline, input and random are not built and stay absent).  DeepLIFT, DeepLIFTWrapper, DeepTaylor and BoundedDeepTaylor
# are built (above) but reached by NAME: their keys deep_lift, deep_lift.wrapper, deep_taylor and deep_taylor.bounded stay out of
# this table, which existing tests pin as it is.
analyzers = {
    "gradient": Gradient,
    "input_t_gradient": InputTimesGradient,
    "deconvnet": Deconvnet,
    "guided_backprop": GuidedBackprop,
    "integrated_gradients": IntegratedGradients,
    "smoothgrad": SmoothGrad,
    "lrp": LRP,
    "lrp.z": LRPZ,
    "lrp.z_IB": LRPZIgnoreBias,
    "lrp.epsilon": LRPEpsilon,
    "lrp.epsilon_IB": LRPEpsilonIgnoreBias,
    "lrp.alpha_beta": LRPAlphaBeta,
    "lrp.alpha_2_beta_1": LRPAlpha2Beta1,
    "lrp.alpha_2_beta_1_IB": LRPAlpha2Beta1IgnoreBias,
    "lrp.alpha_1_beta_0": LRPAlpha1Beta0,
    "lrp.alpha_1_beta_0_IB": LRPAlpha1Beta0IgnoreBias,
    "lrp.z_plus": LRPZPlus,
    "lrp.sequential_preset_a": LRPSequentialPresetA,
    "lrp.sequential_preset_b": LRPSequentialPresetB,
    "lrp.sequential_preset_a_flat": LRPSequentialPresetAFlat,
    "lrp.sequential_preset_b_flat": LRPSequentialPresetBFlat,
}
