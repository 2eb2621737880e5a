"""tests/variant_cases.py reaches what its rows claim -- checked from the table and the built models alone, no GPU: the
parity of every FFT input width, the number of width groups FFTWideStack.refresh forms, the group of `collide` that
holds two row counts, the stack class from_config picks, and that the oracle reads exactly the model's state_dict."""
import pytest
import torch

import variant_cases as V
from oracle import cnf_oracle as O


@pytest.mark.parametrize("name", V.FFT)
def test_fft_case_widths_are_what_the_table_claims(name):
    groups = V.fft_groups(name)
    claimed = V.CASES[name]["widths"]
    assert {n: ("odd" if n % 2 else "even") for n in groups} == claimed
    assert len(groups) == len(claimed)                       # the number of fold GEMMs refresh launches
    # the rfft layout: K = n // 2 + 1 rows each of Re and Im; an odd n has no Nyquist row, so 2 K = n + 1, else n + 2
    for n in groups:
        assert 2 * (n // 2 + 1) == (n + 1 if n % 2 else n + 2)


def test_fft_cases_reach_their_branches():
    assert all(n % 2 for n in V.fft_groups("odd"))                                   # both widths odd
    H = V.CASES["odd"]["nested_sizes"][0]
    assert H == 35 and (H + 1 + 3) // 4 * 4 == 36                          # HP = 36: H + 1 is no multiple of 4
    assert len(V.fft_groups("two_way")) == 3 and not V.CASES["two_way"]["act_norm"]
    assert sorted(set(V.fft_groups("collide")[24])) == [18, 24]                      # one group, two row counts
    assert len(V.fft_groups("collide")) == 1
    assert V.fft_groups("cfg175").keys() == {138, 175}
    assert V.CASES["cfg175"]["nested_sizes"] == [175] * 5 and V.CASES["cfg175"]["dropout"] == 0.407
    assert V.CASES["feat"]["feat"] and V.CASES["glu_feat"]["feat"]
    assert V.CASES["glu_identity"]["activation"] == "Identity" and V.CASES["glu_identity"]["two_way"]


class _Recording(dict):
    """A state dict that records the keys read from it."""

    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


@pytest.mark.parametrize("name", list(V.CASES))
def test_case_builds_the_claimed_stack_and_the_oracle_reads_its_state_dict(name):
    m, spec, sd = V.build(name)
    c = V.CASES[name]
    assert type(m.fused).__name__ == V.STACK_CLASS[c["layer"]]
    if c["layer"] == "LinearFFTEnriched":
        # the model's own bookkeeping agrees with the table: (n, out) per FFT weight, in canonical order
        got = [(n, p.shape[0]) for p, n in zip(m.fused.trainable, m.fused.fft_n) if n is not None]
        assert got == V.fft_weights(name)
        assert all(p.shape[1] == n + 2 * (n // 2 + 1)
                   for p, n in zip(m.fused.trainable, m.fused.fft_n) if n is not None)
    rec = _Recording({k: v.double() for k, v in sd.items()})
    y, cond = V.inputs(name, 3)
    with torch.no_grad():
        h = O.feature_forward(rec, spec, cond.double())
        z, _ = O.model_forward(rec, spec, y.double(), h)
        O.model_inverse(rec, spec, z, h)
    assert rec.read == set(m.state_dict().keys())
    assert torch.isfinite(z).all()
