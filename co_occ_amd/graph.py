"""Serving loop over captured hipGraphs: one host call per stage instead of ~250 launches per sample.

The reference's ``simple_test`` (coocc_ray.py:520-627) is a Python call tree; so was this package's hot path through
round 2, and with the convolutions on the f16 matrix cores (csrc/gemm_h2.hip) the HOST became the bottleneck: ~6 ms of
ctypes launches per sample against ~5 ms of GPU work.  HIP's answer is stream capture: the dense stage of a sample --
G1 gather GEMMs -> con_enc -> CustomResNet3D -> FPN3D -> OccHead (coarse + cascade fine, scattered into the dense grid)
-> render -- is issued ONCE under ``torch.cuda.graph`` and replayed with one ``hipGraphLaunch`` per sample.  What makes the
stage capturable:

* every data-dependent size stays on the device: the non-empty voxel counts of the fuser (``SearchSlot.counts``) and the
  foreground count of the fine branch are read by the kernels themselves (``coocc_conv_desc.M_dev``, the ``*_dev`` entry
  points), grids and buffers are sized for the worst case and surplus workgroups leave at once;
* everything the stage reads sits at fixed addresses: a ``SearchSlot`` per sample in flight (concat rows, voxel lists,
  neighbour tables -- written by the eager search stage on its own stream) and the sample's own tensors.

The index search (K1-K5: FPS chains, top-K, ball query) stays eager on prefetch streams, one sample ahead, exactly as
before: it is latency-bound on two CUs and hidden under the previous sample's dense stage.  A single-modality model
(camera-only ``COOCC_Ray`` with ``occ_fuser=None``, ``COOCC_Ray_L``) has no search: its slot is a ``VoxelSlot`` -- the
frame's voxel volume as rows, filled eagerly (``fill_slot``) -- and the stage starts at the encoder.  Outputs of a replay are the
graph's static tensors (``DenseGraph.out``): valid until the same graph is replayed again.

``tests/test_gpu_graph.py`` checks a replay bit for bit against the eager path on the same sample.
"""
import torch

from . import _lib, core
from .fuser import SearchSlot


NATIVE_SEARCH = __import__("os").environ.get("COOCC_NATIVE_SEARCH", "1") != "0"     # 0: the Python-issued search stage


class DenseGraph:
    """The dense stage of one sample slot as a hipGraph.  ``inputs``: dict(pts [1,C,X,Y,Z], gemo, img_feats, transform) of the
    sample bound to this slot; the slot's concat buffer must have been filled by ``search_into_slot`` at least once before
    capture (warm-up) and before every replay."""

    def __init__(self, model, slot, inputs, stream, render=True):
        self.model, self.slot, self.inputs, self.stream, self.render = model, slot, inputs, stream, render
        self.graph = None
        self.out = None

    def _run(self):
        m, s = self.model, self.inputs
        # single-modality models (coocc_ray.py:255-256: no fuser): the slot's rows ARE the voxel features
        vf = m.occ_fuser.forward_static(self.slot) if m.occ_fuser is not None else self.slot.rows()
        gemo, cam_geo = s.get("gemo"), None
        if self.render and s.get("cams") is not None:
            # P1 per sample (ViewTransformerLSSBEVDepth.py:117-150 via coocc_ray.py:186): the frustum geometry the render
            # block samples comes from the camera matrices inside the stage -- the 39 constants per camera by one tiny kernel,
            # the per-sample chain in the ray kernel itself -- not from a pre-baked [N,D,H,W,3] tensor
            cam_geo = m.img_view_transformer._camera_mats(*s["cams"])
            mats = cam_geo[0].reshape(-1, cam_geo[0].shape[-1])
            cam_geo = (mats,) + tuple(cam_geo[1:])
        return m.decode(vf, gemo, s.get("img_feats"), s.get("transform"), self.render, static=True, cam_geo=cam_geo)

    def capture(self, warmup=2):
        """Eager warm-up on the capture stream (weight packs, per-stream scratch), then the capture itself."""
        assert not core.TIMER.enabled, "kernel timing regions cannot be captured"
        with torch.cuda.stream(self.stream), torch.no_grad():
            for _ in range(warmup):
                self._run()
        self.stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
            self.out = self._run()
        # The captured launches hold RAW pointers into the stream's scratch buffers (Winograd V / M, split-K slabs, arrival
        # counters): keep those tensors alive for as long as the graph exists.  A later eager call on the same stream that
        # needs a larger buffer REPLACES the registry's entry (core.stream_buffer) -- without this reference the old tensor
        # would be freed, handed to someone else by the caching allocator, and every replay would scribble over it.
        dev = self.slot.device
        self._pinned = core.stream_scratch(dev, self.stream)
        for side in core.branch_streams_of(dev, self.stream):          # the stage's forked branches (core.Fork) have their own scratch
            self._pinned += core.stream_scratch(dev, side)
        return self

    def fits(self, counts):
        """Host-side check of a sample's voxel counts against the capacities the graph was captured with."""
        if self.model.occ_fuser is None:          # no voxel lists, no capacity: the stage runs on all V rows
            return True
        Ni, Np = counts
        from . import fuser
        split = fuser.SPLIT_C0 or self.slot.V > fuser.DENSE_C0_MAX_VOXELS
        cap = self.model.occ_fuser.c0_capacity(self.slot.V) if split else self.slot.V   # the dense form of con_enc.0 has no capacity
        return 0 < Np <= cap and Ni > 0

    def replay(self):
        self.graph.replay()
        return self.out


def search_into_slot(model, slot, depth, ctx, cams, pts):
    """Pooling (fused Lift (x) Splat into slot 0 of the slot's concat rows) + index search of one sample on the CURRENT
    stream, outputs in the slot's static buffers.  Returns the ``SearchResult`` (events, host-side counts)."""
    img = model.img_view_transformer.lift_splat(depth, ctx, cams=cams, out=slot.img_rows())
    if NATIVE_SEARCH:
        return model.occ_fuser.search_native(pts, slot)
    return model.occ_fuser.search(img, pts, slot=slot)


class VoxelSlot:
    """The sample slot of a single-modality model (``occ_fuser is None``): one static [V, C] fp32 rows buffer -- the pooled camera
    volume or the LiDAR volume of the frame bound to the slot -- that the captured dense stage reads as its voxel features.  What
    ``SearchSlot`` is to the fused model, without counts, voxel lists or neighbour tables."""

    def __init__(self, C, grid, device):
        X, Y, Z = (int(v) for v in grid)
        C = int(C)
        if min(X, Y, Z, C) <= 0:
            raise ValueError("VoxelSlot: grid %r x %r channels" % (tuple(grid), C))
        self.grid, self.C, self.V = (X, Y, Z), C, X * Y * Z
        self.t = torch.zeros(self.V, C, device=device, dtype=torch.float32)

    @property
    def device(self):
        return self.t.device

    def rows(self):
        X, Y, Z = self.grid
        return core.Rows(self.t, 1, X, Y, Z, self.C, 0, persistent=True)      # rewritten per frame by lift_splat(out=) / fill_volume

    img_rows = rows


def slot_channels(model, example=None):
    """Channels of a single-modality model's voxel features: ``numC_Trans`` of the view transformer, else those of the frame's
    LiDAR volume."""
    vt = getattr(model, "img_view_transformer", None)
    if vt is not None:
        return int(vt.numC_Trans)
    vol = (example or {}).get("pts")
    if vol is None:
        raise ValueError("make_slot: a model without fuser and view transformer takes its channel count from a LiDAR volume (pts)")
    return int(vol.shape[1])


def make_slot(model, grid, device, example=None):
    f = model.occ_fuser
    if f is None:
        return VoxelSlot(slot_channels(model, example), grid, device)
    return SearchSlot(f.in_channels, f.knum, grid, device)


def fill_volume(slot, vol):
    """A [1,C,X,Y,Z] volume (any strides) -> the slot's rows, on the current stream: the layout kernel writing into the static
    buffer, or one flat copy when the volume already is channels-last."""
    r = slot.rows()
    if tuple(vol.shape) != (1, r.C, r.X, r.Y, r.Z):
        raise ValueError("fill_volume: volume %r for a slot of %r" % (tuple(vol.shape), (1, r.C, r.X, r.Y, r.Z)))
    vol = vol.float()
    cl = vol.permute(0, 2, 3, 4, 1)
    if cl.is_contiguous():
        r.t.copy_(cl.reshape(r.V, r.C), non_blocking=True)
    else:
        _lib.call("coocc_ncdhw_to_ndhwc", _lib.ptr(vol.contiguous()), _lib.ptr(r.t), 1, r.C, r.V, r.C, 0)
    return r


def fill_slot(model, slot, fr):
    """The voxel features of one single-modality frame -> the slot's rows on the CURRENT stream (outside the graph: the pooling
    workspace's "left clean" mark lives on a host object, ``ops.pool_ws_clean``, and a capture would freeze it)."""
    if fr.get("depth") is not None:
        model.img_view_transformer.lift_splat(fr["depth"], fr["ctx"], cams=fr["cams"], out=slot.rows())
    elif fr.get("img_voxel_feats") is not None:
        fill_volume(slot, fr["img_voxel_feats"])
    else:
        fill_volume(slot, fr["pts"])
