"""The launch helper's grow-only dynamic-LDS limit (bcnf_rt::launch, bcnf_amd/csrc/bcnf_device.h) inside one process.

Two small-family stacks that differ only in n_conditions run the same kernel instantiations (same nested depth, eval
mode) in the order small, large, small. A limit cached wrongly -- granted for the small request and not raised for
the large one -- comes back as a HIP error status from the large stack's launch (the call raises), not as a fault.

What n_conditions moves: k_forward's request (fwd2_lds_bytes) depends on it only in the pack-free training forward,
so the eval forwards here ask for one size and check that a repeat does not disturb the limit; the backward tail's
request (dw1h_lds_bytes) grows with the padded condition width, 42 KB at C = 16 and 140 KB at C = 208, so the eval
gradients run through the grow path proper. C = 208 is the widest the small family takes (its split-K staging check
in layout_supported admits Cp <= 208; 256 is refused).

Gates: z and log_det_J at the forward gate of tests/test_gpu_parity.py (close(): 1e-5 |ref| + 1e-5 max(1, max|ref|)),
gradients at its gradient gate (rtol 1e-4, floor 1e-4).
"""
import pytest
import torch

from conftest import close
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _stack(C):
    from bcnf_amd import CondRealNVP_v2
    shape = dict(size=19, nested_sizes=[16, 16], n_blocks=2, n_conditions=C, dropout=0.0, act_norm=True)
    torch.manual_seed(100 + C)
    cfg = {"global": {"parameter_selection": [f"p{i}" for i in range(19)]}, "model": {"kwargs": shape},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": C}}]}
    m = CondRealNVP_v2.from_config(cfg)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("scale"):
                p.copy_(0.5 + torch.rand_like(p))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    spec = O.StackSpec(size=19, nested_sizes=[16, 16], n_blocks=2, n_conditions=C, dropout=0.0, act_norm=True)
    cases = {}
    for B in (16, 5):       # a full workgroup of 16 samples and a ragged one
        y, c = torch.randn(B, 19), torch.randn(B, C) / C ** 0.5
        sdg = {k: v.clone().requires_grad_(not k.endswith("orthonormal_matrix")) for k, v in sd.items()}
        cg = c.clone().requires_grad_(True)
        zr, lr = O.model_forward(sdg, spec, y, cg)
        O.inn_nll_loss(zr, lr).backward()
        cases[B] = (y, c, zr.detach(), lr.detach(), cg.grad, {k: v.grad for k, v in sdg.items()})
    return m.to(DEV).eval(), cases


def test_lds_limit_grows_and_stays():
    from bcnf_amd import inn_nll_loss
    small, large = _stack(16), _stack(208)
    for name, (m, cases) in (("small", small), ("large", large), ("small again", small)):
        for B, (y, c, zr, lr, dc, dp) in cases.items():
            m.zero_grad(set_to_none=True)
            cd = c.to(DEV).requires_grad_(True)
            z = m.forward(y.to(DEV), cd, log_det_J=True)      # a failed launch raises with the HIP status
            ok, err = close(z.detach().cpu(), zr)
            assert ok, (name, B, "z", err)
            ok, err = close(m.log_det_J.detach().cpu(), lr)
            assert ok, (name, B, "log_det_J", err)
            inn_nll_loss(z, m.log_det_J).backward()
            ok, err = close(cd.grad.cpu(), dc, rtol=1e-4, floor=1e-4)
            assert ok, (name, B, "dh", err)
            for n, p in m.named_parameters():
                if p.grad is not None:
                    ok, err = close(p.grad.cpu(), dp[n], rtol=1e-4, floor=1e-4)
                    assert ok, (name, B, n, err)
