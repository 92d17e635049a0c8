"""The activation table restated for the tests: the 18 names of the reference's ACTIVATION_FUNCTION
literal, their B2P_ACT_* ids, and every function in float64 torch as transformers' activations.py
defines it (derivatives come from torch.autograd on the restatement). tests/test_act_host.py pins
the restatement to transformers' ACT2FN; this module imports neither transformers nor the reference,
so the GPU tests need neither."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

# name -> id (include/b2p_hip.h)
IDS = {"linear": 0, "gelu": 1, "gelu_python": 1, "silu": 3, "swish": 3,
       "gelu_new": 4, "gelu_fast": 4, "gelu_pytorch_tanh": 4, "gelu_accurate": 4,
       "gelu_10": 5, "quick_gelu": 6, "laplace": 7, "mish": 8, "relu": 9, "relu2": 10, "relu6": 11,
       "sigmoid": 12, "tanh": 13}
NAMES = sorted(IDS)
TANH_GELU_NAMES = ("gelu_new", "gelu_fast", "gelu_pytorch_tanh", "gelu_accurate")
ID_LAST = 13
NEW_IDS = tuple(range(4, ID_LAST + 1))
# the function each id computes on the device ("softsign" is the front end's, not an ACT2FN name)
ID_NAME = {0: "linear", 1: "gelu", 2: "softsign", 3: "silu", 4: "gelu_new", 5: "gelu_10", 6: "quick_gelu",
           7: "laplace", 8: "mish", 9: "relu", 10: "relu2", 11: "relu6", 12: "sigmoid", 13: "tanh"}


def _tanh_gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def _laplace(x, mu=0.707107, sigma=0.282095):
    return 0.5 * (1.0 + torch.erf((x - mu).div(sigma * math.sqrt(2.0))))


FN = {
    "linear": lambda x: x,
    "gelu": F.gelu,
    "gelu_python": lambda x: x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))),
    "silu": F.silu,
    "swish": F.silu,
    "gelu_new": _tanh_gelu,
    "gelu_accurate": _tanh_gelu,
    "gelu_fast": lambda x: 0.5 * x * (1.0 + torch.tanh(x * 0.7978845608 * (1.0 + 0.044715 * x * x))),
    "gelu_pytorch_tanh": lambda x: F.gelu(x, approximate="tanh"),
    "gelu_10": lambda x: torch.clip(F.gelu(x), -10, 10),
    "quick_gelu": lambda x: x * torch.sigmoid(1.702 * x),
    "laplace": _laplace,
    "mish": F.mish,
    "relu": F.relu,
    "relu2": lambda x: torch.square(F.relu(x)),
    "relu6": F.relu6,
    "sigmoid": torch.sigmoid,
    "tanh": torch.tanh,
    "softsign": lambda x: x / (1.0 + x.abs()),
}

KINKS = (0.0, 6.0, 10.0, -10.0)
EXTREMES = (30.0, 88.8, 100.0, 1e4, 1e30)
# value and derivative bound of the kernels against the float64 truth, times max(1, |truth|): the
# longest formula (Mish's derivative) is about eight roundings of at most 2 ulp each
BOUND = 16.0 * 2.0 ** -24


def grid() -> torch.Tensor:
    """1,024 points on [-12, 12] shifted off the kinks, then +-30, +-88.8, +-100, +-1e4, +-1e30: the
    float32 inputs of the kernel tests. Asserts that no point lies within 1e-3 of a kink."""
    x = torch.linspace(-12.0, 12.0 - 0.0117, 1024, dtype=torch.float64) + 0.0117
    ext = torch.tensor([s * v for v in EXTREMES for s in (1.0, -1.0)], dtype=torch.float64)
    x = torch.cat([x, ext]).to(torch.float32)
    assert x.numel() == 1024 + 2 * len(EXTREMES)
    assert float(x[:1024].min()) >= -12.0 and float(x[:1024].max()) <= 12.0
    for k in KINKS:
        assert float((x.double() - k).abs().min()) > 1e-3, k
    return x


def truth(name: str, x32: torch.Tensor):
    """(value, derivative) of the named function at the float32 points x32, in float64."""
    x = x32.detach().double().cpu().clone().requires_grad_(True)
    y = FN[name](x)
    (g,) = torch.autograd.grad(y.sum(), x) if y.requires_grad else (torch.zeros_like(x),)
    return y.detach(), g


def err_ratio(got32: torch.Tensor, want64: torch.Tensor) -> float:
    """max |got - want| / max(1, |want|) over the points whose truth float32 can hold; where it cannot
    (relu2 at 1e30) the result must be the same infinity. No output may be NaN."""
    got = got32.detach().double().cpu()
    assert not torch.isnan(got).any()
    over = want64.abs() > torch.finfo(torch.float32).max
    if over.any():
        assert torch.equal(got[over], torch.sign(want64[over]) * math.inf)
    fin = ~over
    assert torch.isfinite(got[fin]).all()
    return float(((got[fin] - want64[fin]).abs() / want64[fin].abs().clamp_min(1.0)).max())
