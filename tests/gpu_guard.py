"""NaN-guarded device buffers for the GPU tests that drive the C-ABI directly (tests/test_gpu_transformer.py,
tests/test_gpu_linear.py, tests/test_gpu_optim.py): a kernel that writes outside its output kills a canary, one that
leaves part of its output unwritten leaves a NaN inside."""
import torch

DEV = "cuda"
GUARD = 64
NAN = float("nan")


def guarded(rows, width, ld=None, data=None):
    """(buffer, view): a (rows, width) view with row stride ld inside a NaN-filled buffer with GUARD floats either
    side; `data` is copied into the view, everything else stays NaN."""
    ld = width if ld is None else ld
    buf = torch.full((2 * GUARD + rows * ld,), NAN, dtype=torch.float32, device=DEV)
    view = buf[GUARD:GUARD + rows * ld].view(rows, ld)[:, :width]
    if data is not None:
        view.copy_(data)
    return buf, view


INT_CANARY = 0x5A5A5A5A


def guarded1(n, data=None, offset=0, dtype=torch.float32):
    """(buffer, view): n elements of `dtype` starting `offset` elements past the front guard (offset % 4 != 0 takes a
    float view off the 16-byte grid), GUARD elements either side. Floats are NaN-filled, integers INT_CANARY-filled;
    `data` is copied into the view."""
    fill = NAN if dtype.is_floating_point else INT_CANARY
    buf = torch.full((2 * GUARD + offset + n,), fill, dtype=dtype, device=DEV)
    view = buf[GUARD + offset:GUARD + offset + n]
    if data is not None:
        view.copy_(torch.as_tensor(data, dtype=dtype))
    return buf, view


def canaries_alive1(buf, n, offset=0, written=True):
    """guarded1's check: everything outside the view still holds the fill; with `written`, a float view is finite."""
    lo = GUARD + offset
    outside = torch.cat([buf[:lo], buf[lo + n:]])
    if not buf.dtype.is_floating_point:
        return bool((outside == INT_CANARY).all())
    return bool(torch.isnan(outside).all()) and (not written or bool(torch.isfinite(buf[lo:lo + n]).all()))


def canaries_alive(buf, rows, width, ld=None):
    ld = width if ld is None else ld
    outside = torch.ones_like(buf, dtype=torch.bool)
    outside[GUARD:GUARD + rows * ld].view(rows, ld)[:, :width] = False
    inside = buf[~outside]
    return bool(torch.isnan(buf[outside]).all()) and bool(torch.isfinite(inside).all())
