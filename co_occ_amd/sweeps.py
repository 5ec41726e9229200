"""The multi-sweep LiDAR cloud from the raw sweeps.

Four of the five coocc_nusc configs begin their pipeline with ``LoadPointsFromFile(load_dim=5)`` and ``LoadPointsFromMultiSweeps(
sweeps_num=10)``: the key frame and ten earlier sweeps, each moved into the key frame's LiDAR frame, concatenated into the ~280 000-row
cloud that voxelisation, the depth maps and the occupancy loaders then read.  mmdet3d 0.17 does it per sample in numpy -- ten float64
matmuls, ten copies, a concatenation.  Here the raw clouds and a segment table go up through ONE pinned buffer and one asynchronous copy
and csrc/sweeps.hip writes the merged cloud: numpy's float64 arithmetic with its two roundings to fp32, the rows in numpy's order.

mmdet3d is not a dependency; the step is restated from its description (include/coocc_hip.h, ``coocc_sweeps_merge``) and judged
against a numpy restatement the tests carry (tests/sweep_refs.py).

mmdet ``PIPELINES`` run in DataLoader worker processes, which must not open the GPU: ``LoadPointsFromMultiSweeps`` is called in the
main process, as ``image_inputs.LoadMultiViewFrames`` and ``depth_maps.CreateDepthFromLiDAR`` are.
"""
import ctypes
import os

import numpy as np
import torch

from . import _lib, core
from ._lib import ptr, require_gpu
from .staging import HostStage, device_tensor, pinned_upload

# struct coocc_sweep_seg (include/coocc_hip.h), 128 bytes
SEG_DTYPE = np.dtype([("in_row0", "<i8"), ("n_rows", "<i8"), ("out_row0", "<i8"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("dt", "<f4"),
                      ("flags", "<i4")])
TRANSFORM, FILTER = 1, 2          # COOCC_SWEEP_TRANSFORM, COOCC_SWEEP_FILTER
MAX_SWEEPS, MAX_USE = 64, 16      # COOCC_SWEEPS_MAX_SEGS - 1, COOCC_SWEEPS_MAX_USE


def use_columns(use_dim, load_dim):
    """``use_dim`` as mmdet3d reads it (an int ``n`` means ``range(n)``) checked against ``load_dim``: the list of input columns."""
    if int(load_dim) < 5:
        raise ValueError("load_dim must be 5 at least (x y z intensity time: column 4 takes the time lag), got %d" % load_dim)
    cols = list(range(use_dim)) if isinstance(use_dim, (int, np.integer)) else [int(c) for c in use_dim]
    if not 1 <= len(cols) <= MAX_USE:
        raise ValueError("use_dim must name 1 .. %d columns, got %d" % (MAX_USE, len(cols)))
    bad = [c for c in cols if c < 0 or c >= load_dim]
    if bad:
        raise ValueError("use_dim entries %s are outside load_dim = %d" % (bad, load_dim))
    return cols


def choose_sweeps(n, sweeps_num=10, test_mode=False, rng=np.random):
    """The sweeps mmdet3d takes out of ``n``: all of them in order when ``n <= sweeps_num``, the first ``sweeps_num`` in test mode, else
    ``rng.choice(n, sweeps_num, replace=False)`` -- the order drawn is the order of the output."""
    if n <= sweeps_num:
        return np.arange(n)
    if test_mode:
        return np.arange(sweeps_num)
    return np.asarray(rng.choice(n, sweeps_num, replace=False))


def _calibration(sweep, idx):
    R, t = sweep['sensor2lidar_rotation'], sweep['sensor2lidar_translation']
    for name, m, shape in (("sensor2lidar_rotation", R, (3, 3)), ("sensor2lidar_translation", t, (3,))):
        if not isinstance(m, np.ndarray) or m.dtype != np.float64:
            raise ValueError("sweep %d: %s must be a float64 numpy array, got %s (numpy would multiply in another precision; that form "
                             "is not restated)" % (idx, name, getattr(m, "dtype", type(m).__name__)))
        if m.shape != shape:
            raise ValueError("sweep %d: %s must be %s, got %s" % (idx, name, shape, m.shape))
    return R, t


class SweepTable:
    """What ``sweep_table`` returns.  ``segs``: the host records (``SEG_DTYPE``, one per output segment); ``sources``: which cloud every
    part of the raw buffer is (-1 the key frame, else an index into ``sweeps``), in buffer order; ``in_rows``: the rows of the raw buffer;
    ``rows``: the rows of every segment before filtering; ``total``: their sum, the rows of the padded output; ``filtering``: some
    segment drops rows; ``dev``: the records on the device once uploaded (``to``)."""

    def __init__(self, segs, sources, in_rows, filtering):
        self.segs, self.sources, self.in_rows, self.filtering = segs, sources, int(in_rows), bool(filtering)
        self.rows = [int(n) for n in segs["n_rows"]]
        self.total = int(sum(self.rows))
        self.dev = None

    def to(self, device):
        """Upload the records (pinned, asynchronous) unless they are there already."""
        device = torch.device(device)
        require_gpu(device)
        if self.dev is None or self.dev.device != device:
            self.dev = pinned_upload(torch.from_numpy(self.segs.view(np.uint8)), device)[0]
        return self


def sweep_table(points_rows, sweeps, ts, choices, sweep_rows=None, sweeps_num=10, pad_empty_sweeps=False, remove_close=False):
    """The host table of ``coocc_sweeps_merge`` and the layout of its output; opens no GPU.

    ``points_rows``: rows of the key frame.  ``sweeps``: the info dict's list (each entry ``sensor2lidar_rotation`` float64 [3,3],
    ``sensor2lidar_translation`` float64 [3], ``timestamp`` in microseconds).  ``ts``: the sample's timestamp in seconds.  ``choices``:
    indices into ``sweeps`` in output order (``choose_sweeps``).  ``sweep_rows[k]``: rows of ``sweeps[choices[k]]``; by default the
    length of its ``'points'`` entry.  The raw buffer is the key frame followed by the chosen sweeps in that order."""
    if not 0 <= int(sweeps_num) <= MAX_SWEEPS:
        raise ValueError("sweeps_num must be 0 .. %d, got %d" % (MAX_SWEEPS, sweeps_num))
    points_rows = int(points_rows)
    if points_rows < 0:
        raise ValueError("points_rows must be 0 at least, got %d" % points_rows)
    recs = [(0, points_rows, np.zeros(9), np.zeros(3), np.float32(0), 0)]          # the key frame: column 4 = 0, never filtered
    sources, at = [-1], points_rows
    if pad_empty_sweeps and len(sweeps) == 0:
        recs += [(0, points_rows, np.zeros(9), np.zeros(3), np.float32(0), FILTER if remove_close else 0)] * int(sweeps_num)
    else:
        choices = [int(c) for c in choices]
        if len(choices) > MAX_SWEEPS:
            raise ValueError("%d sweeps chosen, %d at most" % (len(choices), MAX_SWEEPS))
        if sweep_rows is not None and len(sweep_rows) != len(choices):
            raise ValueError("sweep_rows has %d entries for %d choices" % (len(sweep_rows), len(choices)))
        for k, idx in enumerate(choices):
            if not 0 <= idx < len(sweeps):
                raise ValueError("choice %d is outside the %d sweeps" % (idx, len(sweeps)))
            sweep = sweeps[idx]
            R, t = _calibration(sweep, idx)
            n = int(sweep_rows[k]) if sweep_rows is not None else len(sweep['points'])
            dt = np.float32(ts - sweep['timestamp'] / 1e6)          # the difference in float64, one rounding
            recs.append((at, n, R.reshape(9), t, dt, TRANSFORM | (FILTER if remove_close else 0)))
            sources.append(idx)
            at += n
    segs = np.zeros(len(recs), SEG_DTYPE)
    out0 = 0
    for s, (in0, n, R, t, dt, flags) in enumerate(recs):
        segs[s] = (in0, n, out0, R, t, dt, flags)
        out0 += n
    if out0 >= 1 << 31 or at >= 1 << 31:
        raise ValueError("%d rows: 2^31 rows and more are not taken" % max(out0, at))
    return SweepTable(segs, sources, at, remove_close and len(recs) > 1)


def merge_sweeps(raw, table, use_dim=(0, 1, 2, 4), radius=1.0, out=None, count=None):
    """The merged cloud of ``raw`` (device fp32 ``[table.in_rows, load_dim]``, every raw cloud back to back) for ``table``
    (``sweep_table``; uploaded here unless ``table.dev`` holds it).  Returns ``(out, count)``.

    Without filtering: ONE launch on the current stream, ``out`` fp32 ``[table.total, len(use_dim)]`` written entirely, ``count`` (int32
    ``[1]`` on the device, optional) = ``table.total``; capturable into a graph with no parallel branches.  With filtering: three
    launches, ``out`` is the padded buffer of which rows ``[0, count)`` are written, ``count`` is made when not given.  Never reads the
    host.  ``out`` and ``count`` are written in place when given.  ``radius``: compared as ``float32(radius)``."""
    raw = device_tensor("raw", raw, torch.float32)
    if raw.shape[0] != table.in_rows:
        raise ValueError("raw must be [%d, load_dim], got %s" % (table.in_rows, tuple(raw.shape)))
    cols = use_columns(use_dim, raw.shape[1])
    dev = raw.device
    if out is None:
        out = torch.empty((table.total, len(cols)), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (table.total, len(cols)) or out.dtype != torch.float32:
        raise ValueError("out must be float32 [%d, %d], got %s %s" % (table.total, len(cols), out.dtype, tuple(out.shape)))
    if count is None and table.filtering:
        count = torch.empty(1, dtype=torch.int32, device=dev)
    elif count is not None and (count.dtype != torch.int32 or count.numel() != 1):
        raise ValueError("count must be int32 [1], got %s %s" % (count.dtype, tuple(count.shape)))
    if table.total == 0:
        if count is not None:
            count.zero_()
        return out, count
    table.to(dev)
    ws = None
    if table.filtering:
        ws = core.stream_buffer(dev, "sweeps", int(_lib.load().coocc_sweeps_merge_ws(table.total)), torch.uint8)
    _lib.call("coocc_sweeps_merge", ptr(raw, torch.float32), table.in_rows, raw.shape[1], ptr(table.dev),
              ctypes.c_void_p(table.segs.ctypes.data), len(table.segs), _lib.host_i32(cols), len(cols), float(np.float32(radius)),
              ptr(out, torch.float32), table.total, ptr(count), ptr(ws), 0 if ws is None else ws.numel())
    return out, count


def read_points(src, load_dim, what="points"):
    """``LoadPointsFromFile``'s read: a path or bytes as ``np.frombuffer(float32).reshape(-1, load_dim)``; a numpy array or a CPU tensor
    is taken as it is (fp32, ``[P, load_dim]``)."""
    if isinstance(src, (str, os.PathLike)):
        src = np.fromfile(src, dtype=np.float32)
    elif isinstance(src, (bytes, bytearray, memoryview)):
        src = np.frombuffer(src, dtype=np.float32)
    elif isinstance(src, torch.Tensor):
        if src.is_cuda:
            raise ValueError("%s is on %s; the loader takes the raw clouds from the host" % (what, src.device))
        src = src.detach().numpy()
    if not isinstance(src, np.ndarray):
        raise ValueError("%s must be a numpy array, a CPU tensor, a path or bytes, got %s" % (what, type(src).__name__))
    if src.dtype != np.float32:
        raise ValueError("%s must be float32, got %s" % (what, src.dtype))
    if src.ndim == 1 and src.size % load_dim == 0:
        src = src.reshape(-1, load_dim)
    if src.ndim != 2 or src.shape[1] != load_dim:
        raise ValueError("%s must be [P, %d], got %s" % (what, load_dim, tuple(src.shape)))
    return src


class LoadPointsFromMultiSweeps:
    """mmdet3d 0.17's LoadPointsFromMultiSweeps (with LoadPointsFromFile's read) on the device; its constructor, plus ``device`` and
    ``rng`` (where the training draw comes from, ``np.random`` as in mmdet3d).  Call it in the main process (it opens the GPU).

    With ``remove_close=False`` a call reads nothing back from the device.  With it, the number of kept rows is only known on the
    device: the call reads the count ONCE to size the returned view, as ``lidar.Voxelization.forward`` reads its voxel count."""

    def __init__(self, sweeps_num=10, load_dim=5, use_dim=[0, 1, 2, 4], pad_empty_sweeps=False, remove_close=False, test_mode=False,
                 device="cuda", rng=np.random):
        self.load_dim = int(load_dim)
        self.use_dim = use_columns(use_dim, self.load_dim)
        if not 0 <= int(sweeps_num) <= MAX_SWEEPS:
            raise ValueError("sweeps_num must be 0 .. %d, got %d" % (MAX_SWEEPS, sweeps_num))
        self.sweeps_num, self.pad_empty_sweeps, self.remove_close, self.test_mode = int(sweeps_num), pad_empty_sweeps, remove_close, test_mode
        self.device, self.rng, self.radius = torch.device(device), rng, 1.0
        self._stage = HostStage(self.device)

    def __call__(self, points, sweeps, timestamp):
        """``points``: the key-frame cloud (a numpy array, a CPU tensor, a path, or bytes); ``sweeps``: the info dict's list, each entry
        ``'data_path'`` or an in-memory ``'points'`` array, ``'sensor2lidar_rotation'``, ``'sensor2lidar_translation'``, ``'timestamp'``;
        ``timestamp``: the sample's, in seconds.  Returns ``(cloud, extras)``: ``cloud`` device fp32 ``[P, len(use_dim)]``; ``extras``
        holds ``choices``, ``rows`` (per segment, before filtering), ``upload_bytes`` and ``count`` (int32 ``[1]`` on the device)."""
        require_gpu(self.device)
        key = read_points(points, self.load_dim)
        padded = self.pad_empty_sweeps and len(sweeps) == 0
        choices = np.arange(0) if padded else choose_sweeps(len(sweeps), self.sweeps_num, self.test_mode, self.rng)
        clouds = [key] + [read_points(sweeps[i]['points'] if 'points' in sweeps[i] else sweeps[i]['data_path'], self.load_dim, "sweep %d" % i)
                          for i in choices]
        table = sweep_table(len(key), sweeps, timestamp, choices, [len(c) for c in clouds[1:]], self.sweeps_num, self.pad_empty_sweeps,
                            self.remove_close)
        raw, table.dev = self._stage([tuple(clouds), table.segs.view(np.uint8)])          # one pinned buffer, one copy
        count = torch.empty(1, dtype=torch.int32, device=self.device)
        out, count = merge_sweeps(raw.view(table.in_rows, self.load_dim), table, self.use_dim, self.radius, count=count)
        cloud = out[:int(_lib.host_read(count)[0])] if table.filtering else out
        return cloud, dict(choices=choices, rows=table.rows, upload_bytes=self._stage.last_bytes, count=count)
