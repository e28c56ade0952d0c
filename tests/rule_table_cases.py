"""The nets, draws and rule tables shared by tests/test_rule_table_ref.py (CPU: the float32 restatement of every draw is within 1e-5
of the float64 one, so the 1e-4 bar of the GPU tests measures the engine and not the draw) and tests/test_gpu_rule_table.py.
Nets and draw construction are those of tests/test_gpu_alphabeta.py (TINY 16 x 16, B = 3; MID 32 x 32, B = 2)."""
import functools

import numpy as np
import torch

import rule_table_ref as RT
from lrp_imagecaptioning_amd.analyzer import rule_table
from lrp_imagecaptioning_amd.synthetic import vgg_weights
from oracle import cnn_lrp_ref as C

TINY_CFG = [("c1", 3, 8, False), ("c2", 8, 8, True), ("c3", 8, 16, False), ("c4", 16, 16, True), ("c5", 16, 16, False)]
MID_CFG = [("c1", 3, 64, False), ("c2", 64, 64, True), ("c3", 64, 128, True), ("c4", 128, 256, False), ("c5", 256, 128, False)]
NETS = {"tiny": (TINY_CFG, 16, 3), "mid": (MID_CFG, 32, 2), "tiny32": (TINY_CFG, 32, 2)}     # tiny32: the narrow net on the 32 x 32 image
BOUNDS = (-124.0, 152.0)                                   # the draws' pixels lie in [-120, 130]
AB10, AB21, EPS = ("alphabeta", 1, 0, True), ("alphabeta", 2, 1, True), ("epsilon", 0.25, True)
EPS_IB, Z, Z_IB = ("epsilon", 0.25, False), ("epsilon", 0.0, True), ("epsilon", 0.0, False)

# name -> (rule, input_layer_rule) as LRP(model, rule=..., input_layer_rule=...) takes them; five convs in both nets
TABLES = {
    "presetAflat": ("Alpha1Beta0", "Flat"),
    "presetBflat": ("Alpha2Beta1", "Flat"),
    "a2b1_ignore_bias": ("Alpha2Beta1IgnoreBias", None),
    "zplus": ("ZPlus", None),
    "presetA_wsquare": ("Alpha1Beta0", "WSquare"),
    "a2b1_bounded": ("Alpha2Beta1", BOUNDS),
    "mixed_ab": ([("alphabeta", 1, 0, True), ("alphabeta", 2, 1, False), ("alphabeta", 1, 0, False), ("alphabeta", 1.5, 0.5, True)], "Flat"),
    "composite": ([AB21, AB21, EPS, EPS], BOUNDS),         # bounded | (2, 1) x lower half | epsilon(0.25) x upper half
    "z": ("Z", None),
    "z_ignore_bias": ("ZIgnoreBias", None),
    "epsilon": (("epsilon", 1e-7, True), None),
    "epsilon_ignore_bias": (("epsilon", 1e-7, False), None),
    # well-conditioned by construction, for the paths the four above cannot reach on the 32 x 32 nets: the bias-free denominator conv
    # at the image layer and on every conv (eps 0.25), the same below a two-chain upper half, and the eps = 0 gates — with the bias
    # (no conv) and without (conv + SafeDivide) — on the layers in the middle, which are the pooled ones of MID
    "eps025_ignore_bias": (EPS_IB, None),
    "eps025_ignore_bias_low": ([EPS_IB, EPS_IB, EPS_IB, AB21, AB21], None),
    "z_middle": ([AB10, Z, Z, Z, AB10], None),
    "z_ignore_bias_pooled": ([AB10, Z_IB, Z_IB, AB10, AB10], None),
}
# The Z / epsilon(1e-7) tables divide by pre-activations that come arbitrarily close to zero, and the float32 restatement of the
# reference's own graph then leaves the float64 one by more than 1e-5 on most draws.  On MID (five convs at 64-256 channels) it does on
# every seed 0 .. 23 tried (1.1e-5 ... 8e-2).  They are checked on TINY at seed 1 (2.9e-6 / 4.1e-6) and, the two with the bias, on
# the 32 x 32 image through the narrow net (tiny32, seed 6: 2.2e-6).  Their IgnoreBias forms meet the condition on no 32 x 32 draw
# tried (tiny32, seeds 0 .. 29: 1.6e-5 ... 5e-3; MID as above): what they run at that size is covered by the eps025 / z_* tables above,
# which pass on both nets (eps025_ignore_bias at seed 10, where MID is 7.1e-6; 1.0e-5 ... 1.4e-5 on seeds 0 .. 9).
Z_FAMILY = ("z", "z_ignore_bias", "epsilon", "epsilon_ignore_bias")
AB_ONLY = ("presetAflat", "presetBflat", "a2b1_ignore_bias", "zplus", "presetA_wsquare", "a2b1_bounded", "mixed_ab")   # fp32 and bf16x3
FP32_ONLY = ("composite", "z", "z_ignore_bias", "epsilon", "epsilon_ignore_bias", "eps025_ignore_bias", "eps025_ignore_bias_low", "z_middle",
             "z_ignore_bias_pooled")
SEED = 7


def seed_of(table_name, net_name="tiny"):
    if table_name in Z_FAMILY:
        return 6 if net_name == "tiny32" else 1
    return 10 if table_name == "eps025_ignore_bias" else SEED


def nets_of(table_name):
    if table_name in ("z", "epsilon"):
        return ("tiny", "tiny32")
    return ("tiny",) if table_name in Z_FAMILY else ("tiny", "mid")


def table(name):
    rule, inp = TABLES[name]
    return rule_table(rule, inp, 5)


@functools.lru_cache(maxsize=None)
def net(name, bias_std=0.3, seed=SEED):
    """weights, images, interleaved token -> image map, relevance maps, layers: computed once per net"""
    cfg, hw, B = NETS[name]
    rs = np.random.RandomState(seed)
    w = vgg_weights(rs, cfg, bias_std=bias_std)
    layers = C.vgg_layers(w, cfg)
    X = rs.uniform(-120, 130, size=(B, hw, hw, 3)).astype(np.float32)
    feat = C.forward(layers, X)
    idx = [b for b in range(B)] + [B - 1 - b for b in range(B)]
    R = (rs.standard_normal((2 * B,) + feat.shape[1:]) * feat[idx]).astype(np.float32)
    return w, X, tuple(idx), R, layers


@functools.lru_cache(maxsize=None)
def refs(net_name, table_name):
    """(float64, float32) restatement for the net's tokens under the table: computed once, never written to"""
    w, X, idx, R, layers = net(net_name, seed=seed_of(table_name, net_name))
    Xi = X[list(idx)]
    t = table(table_name)
    r64, r32 = RT.analyze(layers, Xi, R, t), RT.analyze(layers, Xi, R, t, dtype=torch.float32)
    r64.setflags(write=False); r32.setflags(write=False)
    return r64, r32
