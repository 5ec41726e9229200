"""The one host -> device staging path of the data loaders (image_inputs, depth_maps, occ_gt, sweeps), and the argument checks they
share.  Nothing here opens the GPU before an upload is asked for."""
import numpy as np
import torch

from ._lib import require_gpu


# ------------------------------------------------------------------ checks
def device_tensor(name, t, dtype, cols=None, dim=2):
    """``t`` made contiguous, after checking that it is a device tensor of ``dtype`` with ``dim`` dimensions (and ``cols`` columns)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor, got %s" % (name, type(t).__name__))
    require_gpu(t, name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.dim() != dim or (cols is not None and t.shape[-1] != cols):
        raise ValueError("%s must be %d-dimensional%s, got %s" % (name, dim, "" if cols is None else " with %d columns" % cols, tuple(t.shape)))
    return t.contiguous()


def check_points(points, min_rows=0):
    """``points`` (a tensor or a numpy array, host or device) if it is float32 ``[P >= min_rows, C >= 3]``; ValueError if not."""
    if not isinstance(points, (torch.Tensor, np.ndarray)):
        raise ValueError("points must be a tensor or a numpy array, got %s" % type(points).__name__)
    if points.dtype != (torch.float32 if isinstance(points, torch.Tensor) else np.float32):
        raise ValueError("points must be float32, got %s" % points.dtype)
    if points.ndim != 2 or points.shape[1] < 3 or points.shape[0] < min_rows:
        raise ValueError("points must be [P%s, C >= 3], got %s" % (" >= %d" % min_rows if min_rows else "", tuple(points.shape)))
    return points


def device_points(points, min_rows=0):
    """``check_points`` for a kernel's argument: a device tensor, made contiguous."""
    if not isinstance(points, torch.Tensor):
        raise ValueError("points must be a tensor, got %s" % type(points).__name__)
    require_gpu(points, "points")
    return check_points(points, min_rows).contiguous()


# ------------------------------------------------------------------ uploads
def pinned_upload(host, device):
    """``(device copy, pinned host copy)`` of the CPU tensor ``host``: pinned, then copied asynchronously on the current stream.  For
    tables that go up once; what goes up per sample takes a ``HostStage``."""
    pinned = host.pin_memory()
    return pinned.to(device, non_blocking=True), pinned


_TORCH_DTYPES = {np.dtype(np.uint16): torch.int16}          # torch has no uint16 views; the rest is filled in as it is met


def stage_layout(arrays):
    """The layout of one ``HostStage`` upload; opens no GPU.  ``(parts, shapes, dtypes, offsets, sizes, total)``: per entry of
    ``arrays`` the contiguous numpy arrays that are laid back to back from its offset (one, or the members of a tuple group), the
    shape and the torch dtype of the device view (a group is flat; uint16 is viewed as int16; an empty group is uint8 ``[0]``), its
    byte offset -- a multiple of 256, every entry in a slot of its size rounded up to 256 --, its bytes, and the bytes of the whole
    upload."""
    parts, shapes, dtypes, offs, sizes, at = [], [], [], [], [], 0
    for a in arrays:
        group = isinstance(a, tuple)
        ps = [np.ascontiguousarray(p) for p in a] if group else [np.ascontiguousarray(a)]
        dt = ps[0].dtype if ps else np.dtype(np.uint8)
        if dt not in _TORCH_DTYPES:
            _TORCH_DTYPES[dt] = torch.from_numpy(np.empty(0, dt)).dtype
        n = sum(p.nbytes for p in ps) if group else ps[0].nbytes
        parts.append(ps)
        shapes.append((n // dt.itemsize,) if group else ps[0].shape)
        dtypes.append(_TORCH_DTYPES[dt])
        offs.append(at)
        sizes.append(n)
        at += (n + 255) & ~255
    return parts, shapes, dtypes, offs, sizes, at


class HostStage:
    """Several host arrays (numpy, contiguous or made so, any dtype) -> the device through ONE pinned staging buffer and one
    asynchronous copy: they are laid into the buffer at 256-byte offsets and the device tensors returned are views of that one
    upload (uint16 arrays come back as int16 views of the same bits: torch has no uint16 views).  The buffer grows to the largest
    sample seen and is reused once the previous copy has read it -- a stage WAITS for its previous copy, so independent uploads of
    one call take a stage each.  ``last_bytes``: the bytes of the last upload.

    An entry of ``arrays`` may be a tuple of arrays of one dtype: they are laid BACK TO BACK, with no padding between them, and come
    back as one flat device tensor (``sweeps.LoadPointsFromMultiSweeps``: the raw clouds as one buffer of rows).

    ``threaded_fill``: lay the arrays into the pinned buffer with torch's ``copy_``, which spreads a large array over the host's
    threads, and not with numpy's one thread -- for the camera frames (26 MB: the loader's call takes 0.9 ms, against 1.7 ms through
    numpy); a cloud or a table is there sooner through numpy."""

    def __init__(self, device, threaded_fill=False):
        self.device, self.threaded_fill = torch.device(device), threaded_fill
        self._stage, self._done, self.last_bytes = None, None, 0

    def __call__(self, arrays):
        require_gpu(self.device)
        parts, shapes, dtypes, offs, sizes, at = stage_layout(arrays)
        self.last_bytes = at
        if at == 0:
            return [torch.empty(s, dtype=dt, device=self.device) for s, dt in zip(shapes, dtypes)]
        if self._stage is None or self._stage.numel() < at:
            self._stage = torch.empty(at, dtype=torch.uint8).pin_memory()
        elif self._done is not None:
            self._done.synchronize()                             # the previous sample's copy has read the buffer
        host = self._stage.numpy()
        for ps, o in zip(parts, offs):
            for p in ps:
                flat = p.reshape(-1).view(np.uint8)
                if self.threaded_fill:
                    self._stage[o:o + p.nbytes].copy_(torch.from_numpy(flat))
                else:
                    host[o:o + p.nbytes] = flat
                o += p.nbytes
        dev = self._stage[:at].to(self.device, non_blocking=True)
        self._done = torch.cuda.Event()
        self._done.record()
        return [dev[o:o + n].view(dt).view(s) for s, dt, o, n in zip(shapes, dtypes, offs, sizes)]

    def named(self, host):
        """The same for a dict: its numpy arrays and CPU tensors go up in one staged copy and come back as device tensors under
        their names; device tensors pass through."""
        out = dict(host)
        up = {k: v.detach().numpy() if isinstance(v, torch.Tensor) else v for k, v in host.items()
              if isinstance(v, np.ndarray) or (isinstance(v, torch.Tensor) and not v.is_cuda)}
        if up:
            out.update(zip(up, self(list(up.values()))))
        return out


class PointStage:
    """Host points (a numpy array or a CPU tensor, fp32 ``[P,C]``) -> the device through one pinned staging buffer and one asynchronous
    copy, as the loader uploads frames; device points pass through.  The buffer grows to the largest cloud seen and is reused once the
    previous copy has read it (``HostStage`` with one array)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._host = HostStage(device)

    def __call__(self, points):
        check_points(points)
        if isinstance(points, torch.Tensor) and points.is_cuda:
            return points
        return self._host.named(dict(points=points))["points"]
