"""Case table of the variant coupling stacks (LinearFFTEnriched on the wide kernels through FFTWideStack's fold, AnyGLU
on the layerwise path): the smallest shapes that reach each branch, with the builders the CPU and GPU tests share. Plain
module, no GPU at import. tests/test_variant_cases_cpu.py asserts from this table alone that each case reaches what its
row claims; tests/test_gpu_variants_fp64.py compares each with the fp64 oracle.

FFT cases (layer = "LinearFFTEnriched", GELU). An FFT layer of input width n has K = n // 2 + 1 rfft rows; an odd n
has no Nyquist row. FFTWideStack.refresh / unfold_grad form one GEMM per distinct n over all weights of that width:

  odd      first-layer n = 10 + 13 = 23 odd, hidden n = 35 odd (HP = 36: one padded column)
  two_way  nn_a n = 4 + 6 = 10, nn_b n = 3 + 6 = 9, hidden 33: three width groups, two virtual blocks per block, no
           ActNorm
  collide  first-layer n = 10 + 14 = 24 = hidden n: ONE group holding weights with out = 24 and out = 2 * 9 = 18
  cfg175   trajectory_LSTM_FFT_large_small_cond's own widths (10 + 128 = 138 even, 175 odd) and dropout, two blocks
  feat     behind ConcatenateCondition(90) + FullyConnected([90, 80]), for TrainStep on trajectories

AnyGLU cases (layerwise): glu_odd (odd widths, one-way), glu_identity (g13's shape, two_way, the Identity activation of
trajectory_SFrExp_LSTM_SiGLU_2_large), glu_feat (glu_odd's stack behind the same FullyConnected feature net, C = 80).
"""
import copy
import math

import torch

from oracle import cnf_oracle as O

FEATURE_SIZES = [90, 80]                  # FullyConnected behind ConcatenateCondition(90): trajectories (B, 30, 3)

CASES = {
    # ---- LinearFFTEnriched
    "odd": dict(layer="LinearFFTEnriched", size=19, nested_sizes=[35] * 2, n_conditions=13, n_blocks=2, dropout=0.2,
                B=37, act_norm=True, two_way=False, feat=False,
                widths={23: "odd", 35: "odd"}),
    "two_way": dict(layer="LinearFFTEnriched", size=7, nested_sizes=[33] * 3, n_conditions=6, n_blocks=2, dropout=0.2,
                    B=37, act_norm=False, two_way=True, feat=False,
                    widths={10: "even", 9: "odd", 33: "odd"}),
    "collide": dict(layer="LinearFFTEnriched", size=19, nested_sizes=[24] * 2, n_conditions=14, n_blocks=3, dropout=0.0,
                    B=37, act_norm=True, two_way=False, feat=False,
                    widths={24: "even"}),
    "cfg175": dict(layer="LinearFFTEnriched", size=19, nested_sizes=[175] * 5, n_conditions=128, n_blocks=2,
                   dropout=0.407, B=64, act_norm=True, two_way=False, feat=False,
                   widths={138: "even", 175: "odd"}),
    "feat": dict(layer="LinearFFTEnriched", size=19, nested_sizes=[35] * 2, n_conditions=80, n_blocks=3, dropout=0.3,
                 B=48, act_norm=True, two_way=False, feat=True,
                 widths={90: "even", 35: "odd"}),
    # ---- AnyGLU (layer_kwargs as the reference's run configs: a Sigmoid gate)
    "glu_odd": dict(layer="AnyGLU", glu_activation="Sigmoid", activation="GELU", size=19, nested_sizes=[25] * 2,
                    n_conditions=13, n_blocks=2, dropout=0.2, B=37, act_norm=True, two_way=False, feat=False),
    "glu_identity": dict(layer="AnyGLU", glu_activation="Sigmoid", activation="Identity", size=19,
                         nested_sizes=[24] * 3, n_conditions=12, n_blocks=3, dropout=0.407, B=37, act_norm=True,
                         two_way=True, feat=False),
    "glu_feat": dict(layer="AnyGLU", glu_activation="Sigmoid", activation="GELU", size=19, nested_sizes=[25] * 2,
                     n_conditions=80, n_blocks=2, dropout=0.2, B=37, act_norm=True, two_way=False, feat=True),
}
FFT = [n for n, c in CASES.items() if c["layer"] == "LinearFFTEnriched"]
GLU = [n for n, c in CASES.items() if c["layer"] == "AnyGLU"]
STACK_CLASS = {"LinearFFTEnriched": "FFTWideStack", "AnyGLU": "_LayerwiseStack"}


def fft_weights(name):
    """[(input width n, rows out)] of every LinearFFTEnriched weight of an FFT case in canonical (state_dict) order,
    from the table alone: per block nn_a (input ceil(size / 2) + C), then nn_b (floor(size / 2) + C) when two_way;
    hidden layers H -> H and the final H -> 2 * (the other half)."""
    c = CASES[name]
    da, db = math.ceil(c["size"] / 2), c["size"] // 2
    hs = c["nested_sizes"]
    out = []
    for _ in range(c["n_blocks"]):
        for d_in, d_out in ((da, db), (db, da)) if c["two_way"] else ((da, db),):
            sizes = [d_in + c["n_conditions"]] + list(hs) + [2 * d_out]
            out += list(zip(sizes[:-1], sizes[1:]))
    return out


def fft_groups(name):
    """{n: [out of every weight of input width n]}: the groups FFTWideStack.refresh / unfold_grad form."""
    groups = {}
    for n, out in fft_weights(name):
        groups.setdefault(n, []).append(out)
    return groups


def config(name, dropout=None):
    """The case as CondRealNVP_v2.from_config sees it (dropout: override the table's)."""
    c = CASES[name]
    kw = dict(size=c["size"], nested_sizes=list(c["nested_sizes"]), n_conditions=c["n_conditions"],
              n_blocks=c["n_blocks"], dropout=c["dropout"] if dropout is None else dropout, act_norm=c["act_norm"],
              two_way=c["two_way"], layer=c["layer"], activation=c.get("activation", "GELU"))
    if c["layer"] == "AnyGLU":
        kw["layer_kwargs"] = {"activation": c["glu_activation"]}
    if c["feat"]:
        fnets = [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": FEATURE_SIZES[0]}},
                 {"type": "FullyConnected", "kwargs": {"sizes": list(FEATURE_SIZES), "dropout": 0.0}}]
    else:
        fnets = [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": c["n_conditions"]}}]
    return {"global": {"parameter_selection": [f"p{i}" for i in range(c["size"])]}, "model": {"kwargs": kw},
            "feature_networks": fnets}


def spec(name, dropout=None):
    """The oracle's StackSpec of the case."""
    c = CASES[name]
    return O.StackSpec(size=c["size"], nested_sizes=list(c["nested_sizes"]), n_blocks=c["n_blocks"],
                       n_conditions=c["n_conditions"], dropout=c["dropout"] if dropout is None else dropout,
                       act_norm=c["act_norm"], two_way=c["two_way"],
                       feature_sizes=list(FEATURE_SIZES) if c["feat"] else [], layer=c["layer"],
                       glu_activation=c.get("glu_activation", "GELU"), activation=c.get("activation", "GELU"))


def perturb(m):
    """ActNorm scales in [0.5, 1.5] and ActNorm biases off zero (_perturb of tests/test_gpu_wide.py), and the bias of
    every coupling MLP's first layer moved by 0.1 randn."""
    from test_gpu_train_parity import _perturb
    _perturb(m)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if ".nn.0." in n and n.endswith("bias") and n.startswith("layers."):
                p.add_(0.1 * torch.randn_like(p))


def build(name, dropout=None, seed=7):
    """(model on the CPU, oracle spec, fp32 state dict): torch.manual_seed init, then `perturb`. No GPU."""
    from bcnf_amd import CondRealNVP_v2
    torch.manual_seed(seed)
    m = CondRealNVP_v2.from_config(copy.deepcopy(config(name, dropout)))
    perturb(m)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m, spec(name, dropout), sd


def inputs(name, B=None):
    """(y, condition) of the case at B rows (default: the table's): trajectories (B, 30, 3) behind the feature net."""
    c = CASES[name]
    B = c["B"] if B is None else B
    g = torch.Generator().manual_seed(3000 + B)
    y = torch.randn(B, c["size"], generator=g)
    cond = torch.randn(B, 30, 3, generator=g) if c["feat"] else torch.randn(B, c["n_conditions"], generator=g)
    return y, cond
