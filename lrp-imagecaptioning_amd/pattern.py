"""PatternComputer (innvestigate/tools/pattern.py:344-) for the VGG-style encoders: the patterns of every conv of an
ImageModelSpec from data, accumulated and computed on the device (LRPEngine.pattern_fit_*).

    patterns = PatternComputer(spec, pattern_type="relu").compute(X, batch_size=32)     # one (3, 3, cin, cout) array per conv
    PatternNet(spec, patterns=patterns).analyze([X, head])

One pattern type returns the list, several a dict type -> list, as the reference does.  Each type is one pass over the data."""
import numpy as np

from .engine import LRPEngine

PATTERN_TYPES = ("linear", "relu", "relu.positive", "relu.negative")


def fit_engine(engine, batches, pattern_type):
    """One fit on `engine` over an iterable of batches (arrays (B, H, W, 3), or lists holding one); batches larger than the
    engine's max_images are cut.  Returns the patterns."""
    engine.pattern_fit_begin(pattern_type)
    seen = 0
    for Xs in batches:
        x = np.asarray(Xs[0] if isinstance(Xs, (list, tuple)) else Xs, dtype=np.float32)
        for lo in range(0, len(x), engine.max_images):
            engine.encode_images(x[lo:lo + engine.max_images])
            engine.pattern_fit_batch()
            seen += 1
    if not seen:
        raise ValueError("the pattern fit needs at least one image")
    engine.pattern_fit_end()
    return engine.get_patterns()


class PatternComputer(object):
    def __init__(self, model, pattern_type="linear", compute_layers_in_parallel=True, gpus=None, max_batch=32, device=None):
        if getattr(model, "resnet", None) is not None:
            raise Exception("Model contains not supported layer: BatchNormalization / Add (a ResNet encoder)")    # :369-373
        types = list(pattern_type) if isinstance(pattern_type, (list, tuple)) else [pattern_type]
        for t in types:
            if t not in PATTERN_TYPES:
                raise ValueError("unknown pattern type %r: one of %s" % (t, list(PATTERN_TYPES)))
        self.model = model
        self.pattern_types = types
        self.compute_layers_in_parallel = compute_layers_in_parallel
        self.gpus = gpus
        if self.compute_layers_in_parallel is False:
            raise NotImplementedError("Not supported.")                                                           # :381-382
        if gpus is not None and gpus > 1:
            raise NotImplementedError("Not supported yet.")                                                       # :447-448
        self._max_batch, self._device = int(max_batch), device
        self._engine = None

    def _get_engine(self):
        if self._engine is None:
            m = self.model
            h, w, c = m.output_shape()
            self._engine = LRPEngine(decoder="adaptive", cnn_cfg=m.cnn_cfg, img_hw=m.img_hw, L=h * w, D=c, H=8, E=8, V=4,
                                     max_images=self._max_batch, max_tokens=self._max_batch, max_caption_len=2, device=self._device)
            self._engine.set_weights(m.weights)
            self._engine.set_precision("fp32")
        return self._engine

    def compute(self, X, batch_size=32, verbose=0):
        X = np.asarray(X, dtype=np.float32)
        return self.compute_generator(lambda: (X[lo:lo + batch_size] for lo in range(0, len(X), batch_size)))

    def compute_generator(self, generator, **kwargs):
        """generator: a callable returning an iterable of batches (called once per pattern type), or an iterable that can be
        walked once per type (a list, a Sequence)."""
        if "epochs" in kwargs and kwargs["epochs"] != 1:
            raise ValueError("Pattern are computed with a closed form solution. Only need to do one epoch.")      # :478-481
        if not callable(generator) and len(self.pattern_types) > 1 and iter(generator) is generator:
            raise ValueError("several pattern types take one pass over the data each: pass a callable or a re-iterable")
        eng = self._get_engine()
        patterns = {t: fit_engine(eng, generator() if callable(generator) else generator, t) for t in self.pattern_types}
        return patterns[self.pattern_types[0]] if len(self.pattern_types) == 1 else patterns
