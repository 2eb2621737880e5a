"""What notebooks/resimulation.ipynb (psaegert/bcnf) computes from the re-simulated positions, on the device.

The notebook's chain is sample -> resimulate -> analyse. Its only use of X_resim (N, M, S, 3) is to reduce it over the
draw axis to two small results:

  * the resimulation error  X_errors = np.nanmedian(np.nanmean((X_resim - X[:, None])**2, axis=3), axis=1)   (N, S);
  * the impacts  np.where(np.diff((X_resim[i, :, :, -1] > 0).astype(int), axis=1) == -1)  per trajectory i, the
    positions at those (draw, step) pairs and one hist2d of them over np.linspace(-42, 42, 128).

`resimulation_error_device` and `impacts_device` are those reductions as HIP kernels (bcnf_amd/csrc/
bcnf_resim_stats.hip) on the positions `resimulate_device` leaves in HBM; `resimulation_error_host` and `impacts_host`
are the numpy statements themselves (the oracle of the tests: the kernels return the same bits). `resimulation_summary`
runs the whole chain one slice of trajectories at a time, so the positions never leave the device and only one slice
of them is ever resident.

An impact's step is the np.diff index: the LAST step still above ground (z[s] > 0 and not z[s + 1] > 0; NaN is not
above, as in numpy). A draw can have more than one (thrust can lift a ball again): `step` / `position` are the first,
`transitions` counts them and the histogram holds every one, as the notebook's np.where lists every one.

One deviation from numpy, in `resimulation_error_device` only: for an odd number of non-NaN draws and M < 600 numpy's
small-array nanmedian returns (v + v) / 2, which overflows to inf for v > DBL_MAX / 2; the kernel returns v.
"""
from __future__ import annotations

import warnings

import numpy as np
import torch

from . import _native
from .resimulation import _warn_unfinished, resimulate_device, time_grid

MAX_DRAWS = _native.RESIM_ERROR_MAX_DRAWS      # one column of draws is sorted in a workgroup's LDS
MAX_EDGES = _native.RESIM_HIST_MAX_EDGES       # the (E - 1)^2 counters of one trajectory live in a workgroup's LDS
SLICE_BYTES = 256 * 1024 * 1024                # resimulation_summary: positions of one slice of trajectories, at most
DEFAULT_BINS = np.linspace(-42, 42, 128)       # the notebook's hist2d edges


# ---------------------------------------------------------------------------------------------------------- host
def resimulation_error_host(x, observed) -> np.ndarray:
    """np.nanmedian(np.nanmean((x - observed[:, None])**2, axis=3), axis=1): (N, S) float64 for x (N, M, S, 3) and
    observed (N, S, 3) (the notebook's X_errors)."""
    x = np.asarray(x, dtype=np.float64)
    observed = np.asarray(observed).astype(np.float64)
    _check_shapes(x.shape, observed.shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)       # "Mean of empty slice" / "All-NaN slice"
        with np.errstate(all="ignore"):
            return np.nanmedian(np.nanmean((x - observed[:, None]) ** 2, axis=3), axis=1)


def impacts_host(x, bins=None) -> dict:
    """The notebook's impact expressions on x (N, M, S, 3). `indices[i]` is its list form, the (draw, step) index
    arrays of np.where(np.diff((x[i, :, :, -1] > 0).astype(int), axis=1) == -1); `step`, `position`, `transitions`
    and `hist` are what `impacts_device` returns, derived from it: the first step per draw (-1: none) and the position
    there (NaN: none), the number of steps per draw, and np.histogram2d of every listed position's (x, y) over `bins`
    for both axes, (N, E - 1, E - 1) int32 (None without bins)."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 4 or x.shape[3] != 3:
        raise ValueError(f"x must be (N, M, S, 3), got shape {x.shape}")
    n, m = x.shape[:2]
    edges = None if bins is None else _edges(bins)
    step = np.full((n, m), -1, dtype=np.int32)
    position = np.full((n, m, 3), np.nan)
    transitions = np.zeros((n, m), dtype=np.int32)
    hist = None if edges is None else np.zeros((n, len(edges) - 1, len(edges) - 1), dtype=np.int32)
    indices = []
    for i in range(n):
        draw, s = np.where(np.diff((x[i, :, :, -1] > 0).astype(int), axis=1) == -1)
        indices.append((draw, s))
        which, first, count = np.unique(draw, return_index=True, return_counts=True)    # np.where lists row-major
        step[i, which] = s[first]
        transitions[i, which] = count
        hit = step[i] >= 0
        position[i, hit] = x[i, hit, step[i, hit]]
        if hist is not None:
            pos = x[i, draw, s]
            # [edges, edges]: a bare table of two edges would be read as the bin COUNTS of the two axes
            hist[i] = np.histogram2d(pos[:, 0], pos[:, 1], bins=[edges, edges])[0].astype(np.int32)
    return {"step": step, "position": position, "transitions": transitions, "hist": hist, "indices": indices}


# -------------------------------------------------------------------------------------------------------- checks
def _check_shapes(xs, os_) -> None:
    if len(xs) != 4 or xs[3] != 3:
        raise ValueError(f"x must be (N, M, S, 3), got shape {tuple(xs)}")
    if len(os_) != 3 or os_[2] != 3:
        raise ValueError(f"observed must be (N, S, 3), got shape {tuple(os_)}")
    if os_[0] != xs[0] or os_[1] != xs[2]:
        raise ValueError(f"observed has shape {tuple(os_)}, x {tuple(xs)} needs ({xs[0]}, {xs[2]}, 3)")
    if xs[2] < 1:
        raise ValueError(f"x must hold at least one time step, got shape {tuple(xs)}")


def _edges(bins) -> np.ndarray:
    edges = np.ascontiguousarray(np.asarray(bins, dtype=np.float64))
    if edges.ndim != 1 or edges.size < 2:
        raise ValueError(f"bins must be a 1-D table of at least 2 edges, got shape {edges.shape}")
    if not (np.diff(edges) > 0).all():
        raise ValueError("bins must increase strictly")
    return edges


def _device_positions(x) -> torch.Tensor:
    if not x.is_cuda:
        raise RuntimeError("bcnf_amd resimulation statistics run on the HIP device only (no CPU path): x must be a "
                           "device tensor, as resimulate_device returns it; got " + str(x.device))
    return x.contiguous()


def _positions(x) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"x must be a torch tensor (resimulate_device's positions), got {type(x).__name__}")
    if x.dtype != torch.float64:
        raise ValueError(f"x must be float64 (resimulate_device's positions), got {x.dtype}")
    return x


# -------------------------------------------------------------------------------------------------------- device
def resimulation_error_device(x: torch.Tensor, observed) -> torch.Tensor:
    """`resimulation_error_host` on the device, the same bits: (N, S) float64 device tensor for positions x
    (N, M, S, 3) float64 on the device and observed (N, S, 3) (tensor or numpy; float32 and float64 are read as they
    are, anything else is converted to float64). M <= MAX_DRAWS (16384), else ValueError. Deviation: for an odd
    number of non-NaN draws numpy's path for M < 600 computes (v + v) / 2, inf for v > DBL_MAX / 2; this returns v."""
    x = _positions(x)
    obs = torch.as_tensor(observed)
    _check_shapes(x.shape, obs.shape)
    n, m, s, _ = x.shape
    if m > MAX_DRAWS:
        raise ValueError(f"resimulation_error_device sorts one column of draws in a workgroup's LDS: at most "
                         f"{MAX_DRAWS} draws, got {m}")
    x = _device_positions(x)
    if obs.dtype not in (torch.float32, torch.float64):
        obs = obs.to(torch.float64)
    obs = obs.to(x.device).contiguous()
    if m == 0:
        return torch.full((n, s), float("nan"), dtype=torch.float64, device=x.device)
    err = torch.empty((n, s), dtype=torch.float64, device=x.device)
    if n:
        with torch.cuda.device(x.device):
            _native.call("bcnf_resim_error_median", x, obs, obs.dtype == torch.float64, n, m, s, err,
                         _native.stream_handle(x.device))
    return err


def impacts_device(x: torch.Tensor, bins=None) -> dict:
    """`impacts_host` on the device (without the list form): dict of device tensors `step` (N, M) int32, `position`
    (N, M, 3) float64, `transitions` (N, M) int32 and `hist` (N, E - 1, E - 1) int32 for E = len(bins) edges (None
    without bins). E <= MAX_EDGES (192), else ValueError."""
    x = _positions(x)
    if x.ndim != 4 or x.shape[3] != 3 or x.shape[2] < 1:
        raise ValueError(f"x must be (N, M, S, 3) with S >= 1, got shape {tuple(x.shape)}")
    n, m, s, _ = x.shape
    edges = None if bins is None else _edges(bins.detach().cpu().numpy() if isinstance(bins, torch.Tensor) else bins)
    if edges is not None and edges.size > MAX_EDGES:
        raise ValueError(f"impacts_device keeps one trajectory's histogram in a workgroup's LDS: at most {MAX_EDGES} "
                         f"edges, got {edges.size}")
    x = _device_positions(x)
    dev = x.device
    step = torch.empty((n, m), dtype=torch.int32, device=dev)
    position = torch.empty((n, m, 3), dtype=torch.float64, device=dev)
    transitions = torch.empty((n, m), dtype=torch.int32, device=dev)
    hist = edges_d = None
    if edges is not None:      # the kernel writes hist[i] whole; no trajectory or no draw: nothing is launched
        hist = (torch.empty if n * m else torch.zeros)((n, edges.size - 1, edges.size - 1), dtype=torch.int32,
                                                       device=dev)
        edges_d = torch.from_numpy(edges).to(dev)
    if n * m:
        with torch.cuda.device(dev):
            _native.call("bcnf_resim_impacts", x, n, m, s, edges_d, 0 if edges is None else edges.size, step, position,
                         transitions, hist, _native.stream_handle(dev))
    return {"step": step, "position": position, "transitions": transitions, "hist": hist}


def default_chunk_trajectories(m: int, steps: int, limit: int = SLICE_BYTES) -> int:
    """Trajectories per slice so that the slice's positions (chunk x M x steps x 3 float64) stay within `limit` bytes
    (256 MiB); one trajectory at least."""
    return max(1, limit // max(1, m * steps * 24))


def resimulation_summary(model, T, dt: float, data_dict: dict, y_hat=None, *conditions: torch.Tensor, observed,
                         m_samples: int = 1000, break_on_impact: bool = False, batch_size: int = 100,
                         bins=DEFAULT_BINS, chunk_trajectories: int | None = None, verbose: bool = True) -> dict:
    """sample -> resimulate -> analyse without the positions leaving the device: `resimulate`'s arguments plus the
    observed trajectories (N, S, 3), S = len(np.arange(0, T, dt)). The draws are taken (y_hat (M, N, D)) or drawn
    exactly as `resimulate` does, so the same seed gives the same draws. The trajectories are walked in slices of
    `chunk_trajectories` (default: `default_chunk_trajectories`, the slice's positions within 256 MiB): per slice one
    `resimulate_device` launch, the two reductions, and the positions are dropped. The result does not depend on the
    slicing. Returns numpy arrays:
      errors (N, S)                        the notebook's X_errors
      impact_step (N, M) int32             first np.diff index per draw, -1 = none
      impact_position (N, M, 3)            the position there, NaN = none
      impact_transitions (N, M) int32      how many per draw
      impact_hist (N, E - 1, E - 1) int32  np.histogram2d of every impact's (x, y) per trajectory (None: bins=None)
      observed_impact_step (N,), observed_impact_position (N, 3)   the same expression on the observed trajectories
      status_counts (3,) int64             draws with BCNF_RESIM_OK / _NONFINITE / _STEPS
    Unfinished trajectories give `resimulate`'s RuntimeWarning."""
    if y_hat is None:
        if len(conditions) != model.feature_network_stack.n_distinct_conditions:
            raise ValueError(f"Expected {model.feature_network_stack.n_distinct_conditions} conditions, "
                             f"got {len(conditions)}")
        y_hat = model.sample(m_samples, *conditions, batch_size=batch_size, verbose=verbose, outer=True,
                             output_device=model.device)
    yt = torch.as_tensor(y_hat)
    if yt.ndim != 3:
        raise ValueError(f"y_hat must be (M, N, D), got shape {tuple(yt.shape)}")
    M, N = int(yt.shape[0]), int(yt.shape[1])
    steps = len(time_grid(T, dt))
    if steps == 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    obs = torch.as_tensor(observed)
    _check_shapes((N, M, steps, 3), obs.shape)
    if M > MAX_DRAWS:
        raise ValueError(f"resimulation_summary sorts one column of draws in a workgroup's LDS: at most {MAX_DRAWS} "
                         f"draws, got {M}")
    edges = None if bins is None else _edges(bins)
    if edges is not None and edges.size > MAX_EDGES:
        raise ValueError(f"resimulation_summary keeps one trajectory's histogram in a workgroup's LDS: at most "
                         f"{MAX_EDGES} edges, got {edges.size}")
    if chunk_trajectories is None:
        chunk_trajectories = default_chunk_trajectories(M, steps)
    chunk_trajectories = int(chunk_trajectories)
    if chunk_trajectories < 1:
        raise ValueError(f"chunk_trajectories must be at least 1, got {chunk_trajectories}")
    if verbose:
        print(f"Resimulating {N} trajectories {M} times")
    device = torch.device(model.device)                 # as resimulate: a model on the CPU still runs on the GPU
    if device.type != "cuda":
        device = yt.device if yt.is_cuda else torch.device("cuda", torch.cuda.current_device())
    if yt.dtype not in (torch.float32, torch.float64):
        yt = yt.to(torch.float64)
    yt = yt.to(device)
    if obs.dtype not in (torch.float32, torch.float64):
        obs = obs.to(torch.float64)
    obs = obs.to(device).contiguous()
    nb = 0 if edges is None else edges.size - 1
    out = {"errors": np.full((N, steps), np.nan),
           "impact_step": np.full((N, M), -1, dtype=np.int32),
           "impact_position": np.full((N, M, 3), np.nan),
           "impact_transitions": np.zeros((N, M), dtype=np.int32),
           "impact_hist": None if edges is None else np.zeros((N, nb, nb), dtype=np.int32)}
    status_counts = torch.zeros(3, dtype=torch.int64, device=device)
    if M:
        for a in range(0, N, chunk_trajectories):
            b = min(N, a + chunk_trajectories)
            dd = {k: v[a:b] for k, v in data_dict.items()}
            x, _, status = resimulate_device(yt[:, a:b], T, dt, dd, model.parameter_index_mapping,
                                             break_on_impact=break_on_impact, device=device, return_status=True)
            err = resimulation_error_device(x, obs[a:b])
            imp = impacts_device(x, edges)
            del x                                     # the slice's positions go back to the allocator here
            status_counts += torch.bincount(status.reshape(-1).to(torch.int64).clamp_(0, 2), minlength=3)
            out["errors"][a:b] = err.cpu().numpy()
            out["impact_step"][a:b] = imp["step"].cpu().numpy()
            out["impact_position"][a:b] = imp["position"].cpu().numpy()
            out["impact_transitions"][a:b] = imp["transitions"].cpu().numpy()
            if edges is not None:
                out["impact_hist"][a:b] = imp["hist"].cpu().numpy()
    counts = status_counts.cpu().numpy()
    if counts[2]:                                     # resimulate's warning, from the counts of all slices
        status_all = torch.zeros(N * M, dtype=torch.int32)
        status_all[:int(counts[2])] = 2
        _warn_unfinished(status_all)
    oimp = impacts_device(obs.to(torch.float64)[:, None].contiguous())
    out["observed_impact_step"] = oimp["step"][:, 0].cpu().numpy()
    out["observed_impact_position"] = oimp["position"][:, 0].cpu().numpy()
    out["status_counts"] = counts
    return out


__all__ = ["resimulation_error_device", "resimulation_error_host", "impacts_device", "impacts_host",
           "resimulation_summary", "default_chunk_trajectories", "MAX_DRAWS", "MAX_EDGES", "SLICE_BYTES"]
