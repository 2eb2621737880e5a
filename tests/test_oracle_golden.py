"""Pin the CPU oracle (oracle/cnf_oracle.py) against fixtures produced by running the reference itself."""
import numpy as np
import pytest
import torch

from conftest import close, golden_sd, load_golden
from oracle import cnf_oracle as O


def test_oracle_forward_matches_reference(g1):
    sd = golden_sd(g1)
    y, traj = torch.from_numpy(g1["y"]), torch.from_numpy(g1["traj"])
    h = O.feature_forward(sd, O.FC_SMALL_SPEC, traj)
    assert close(h, g1["h"], rtol=1e-6, floor=1e-6)[0]
    z, ldj = O.model_forward(sd, O.FC_SMALL_SPEC, y, h)
    ok, err = close(z, g1["z"], rtol=1e-6, floor=1e-6)
    assert ok, err
    assert close(ldj, g1["ldj"], rtol=1e-6, floor=1e-6)[0]
    assert close(O.inn_nll_loss(z, ldj, "none"), g1["nll"], rtol=1e-6, floor=1e-6)[0]


def test_oracle_inverse_matches_reference(g1):
    sd = golden_sd(g1)
    traj = torch.from_numpy(g1["traj"])
    h = O.feature_forward(sd, O.FC_SMALL_SPEC, traj)
    inv = O.model_inverse(sd, O.FC_SMALL_SPEC, torch.from_numpy(g1["zr"]), h)
    ok, err = close(inv, g1["inv_zr"], rtol=1e-6, floor=1e-6)
    assert ok, err


def test_oracle_grads_match_reference(g1):
    sd = {k: v.clone().requires_grad_(not k.endswith("orthonormal_matrix")) for k, v in golden_sd(g1).items()}
    y, traj = torch.from_numpy(g1["y"]), torch.from_numpy(g1["traj"])
    h = O.feature_forward(sd, O.FC_SMALL_SPEC, traj)
    h.retain_grad()
    z, ldj = O.model_forward(sd, O.FC_SMALL_SPEC, y, h)
    O.inn_nll_loss(z, ldj).backward()
    assert close(h.grad, g1["dh"], rtol=1e-5, floor=1e-6)[0]
    for k in g1.keys():
        if k.startswith("grad/"):
            name = k[5:]
            ok, err = close(sd[name].grad, g1[k], rtol=1e-5, floor=1e-6)
            assert ok, (name, err)


def test_oracle_sample_matches_reference(g1):
    d = load_golden("g3_sample.npz")
    sd = golden_sd(g1)
    traj = torch.from_numpy(d["traj"])
    torch.manual_seed(2024_03_25 + 4)
    s = O.sample(sd, O.FC_SMALL_SPEC, 500, traj, outer=True, batch_size=100)
    ok, err = close(s, d["sample"], rtol=1e-6, floor=1e-6)
    assert ok, err
    torch.manual_seed(2024_03_25 + 5)
    s2 = O.sample(sd, O.FC_SMALL_SPEC, 250, traj, outer=True, batch_size=3, sample_batch_size=64)
    assert close(s2, d["sample2"], rtol=1e-6, floor=1e-6)[0]


def test_oracle_two_way_matches_reference():
    d = load_golden("g6_two_way.npz")
    sd = {k[len("layer_sd/"):]: torch.from_numpy(d[k]) for k in d.keys() if k.startswith("layer_sd/")}
    spec = O.StackSpec(size=7, nested_sizes=[19] * 5, n_blocks=1, n_conditions=5, two_way=True)
    sd = {"layers.0." + k: v for k, v in sd.items()}
    z, ldj = O.coupling_forward(sd, "layers.0", spec, torch.from_numpy(d["x"]), torch.from_numpy(d["c"]))
    assert close(z, d["z"], 1e-6, 1e-6)[0] and close(ldj, d["ldj"], 1e-6, 1e-6)[0]
    inv = O.coupling_inverse(sd, "layers.0", spec, z, torch.from_numpy(d["c"]))
    assert close(inv, d["inv"], 1e-6, 1e-6)[0]
    # the two_way "inverse" is not the inverse: the reference's own round trip error is large
    assert float((inv - torch.from_numpy(d["x"])).abs().max()) > 1e-4


VARIANT_FIXTURES = {
    "g12_fft_enriched.npz": O.StackSpec(size=19, nested_sizes=[40] * 3, n_blocks=3, n_conditions=12, dropout=0.407,
                                        act_norm=True, layer="LinearFFTEnriched"),
    "g13_anyglu.npz": O.StackSpec(size=19, nested_sizes=[24] * 3, n_blocks=3, n_conditions=12, dropout=0.407,
                                  act_norm=True, two_way=True, layer="AnyGLU", glu_activation="Sigmoid"),
}


@pytest.mark.parametrize("fixture", sorted(VARIANT_FIXTURES))
def test_oracle_variant_layers_match_reference(fixture):
    """The oracle's LinearFFTEnriched (torch.fft.rfft, not the package's rfft matrix) and AnyGLU layers in float64
    against the reference's own eval-mode outputs and autograd gradients (g12: FFT, one-way; g13: AnyGLU with a
    Sigmoid gate, two_way, the bug-compatible inverse included): z, ldj, inverse, loss and every grad/* entry at this
    file's gate without its relative term, |err| <= 1e-6 max(1, max|ref|). The fixtures are fp32 results, so what is
    left is their own rounding: z 1.9e-7 / 1.7e-7, ldj 1.2e-7, inverse 1.7e-7 / 2.6e-7, worst gradient 1.4e-7 /
    1.6e-7 of that scale."""
    d = load_golden(fixture)
    spec = VARIANT_FIXTURES[fixture]
    sd = {k: v.double().requires_grad_(not k.endswith("orthonormal_matrix")) for k, v in golden_sd(d).items()}
    y, c = torch.from_numpy(d["y"]).double(), torch.from_numpy(d["cond"]).double()
    z, ldj = O.model_forward(sd, spec, y, c)
    loss = O.inn_nll_loss(z, ldj)
    loss.backward()
    with torch.no_grad():
        inv = O.model_inverse(sd, spec, torch.from_numpy(d["z"]).double(), c)
    for key, got in (("z", z), ("ldj", ldj), ("inv", inv), ("loss", loss)):
        ok, err = close(got.detach(), d[key], rtol=0.0, floor=1e-6)
        assert ok, (fixture, key, err)
    grads = [k for k in d.keys() if k.startswith("grad/")]
    assert sorted(k[5:] for k in grads) == sorted(k for k, v in sd.items() if v.requires_grad)
    for k in grads:
        ok, err = close(sd[k[5:]].grad, d[k], rtol=0.0, floor=1e-6)
        assert ok, (fixture, k, err)


def test_orthonormal_regeneration_bit_exact_on_this_host():
    """Q = qr(randn(19,19))[0] after manual_seed is bit-identical to the reference on the same host/LAPACK.
    (On another CPU the LAPACK path may differ by an ulp — the reference itself is not portable there;
    checkpoints carry Q and load bit-exactly, see tests/test_gpu_parity.py.)"""
    from bcnf_amd import OrthonormalTransformation
    d = load_golden("g8_q.npz")
    q = OrthonormalTransformation(19, random_state=2024_03_25).orthonormal_matrix.detach().numpy()
    if q.tobytes() != d["q"].tobytes():
        import pytest
        assert np.abs(q - d["q"]).max() < 1e-6
        pytest.skip("LAPACK on this host rounds differently from the fixture host (ulp-level)")


def test_init_state_dict_bit_exact_vs_reference():
    """from_config under torch.manual_seed consumes the CPU RNG in the reference's order (cnf.py:395-423)."""
    from bcnf_amd import CondRealNVP_v2
    from conftest import FC_SMALL_CFG as FC_SMALL
    d = load_golden("g_init.npz")
    torch.manual_seed(2024_03_25)
    m = CondRealNVP_v2.from_config(FC_SMALL)
    sd = m.state_dict()
    assert set("sd/" + k for k in sd) == set(d.keys())
    for k, v in sd.items():
        if k.endswith("orthonormal_matrix"):
            assert np.abs(v.numpy() - d["sd/" + k]).max() < 1e-6
        else:
            assert np.array_equal(v.numpy(), d["sd/" + k]), k
