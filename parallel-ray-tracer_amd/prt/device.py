"""Device mirror of the render seam over librt_hip.so (include/rt_hip.h):
load_to_gpu -> Renderer.upload, render_frame -> Renderer.render, load_from_gpu -> Renderer.download.

No fallback: if librt_hip.so is missing or no GPU is visible, constructing a Renderer raises.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import BvhNode, Camera, Frame, Light, Opts, SceneDesc, Stats, Triangle, Vec3

P = ctypes.POINTER

KERNELS = {"auto": 0, "strict": 1, "fast": 2}
# rt_frame.variant (launch configurations of the fast kernel, include/rt_hip.h); a variant name is also
# accepted as `kernel` (kernel="coop4" == kernel="fast", variant="coop4")
VARIANTS = {"default": 0, "persist": 1, "persist4": 2, "coop2": 4, "coop4": 5, "hybrid": 11, "shpool": 13, "shdefer": 15}
VARIANT_NAMES = {v: k for k, v in VARIANTS.items()}
HOT_KERNELS = {"coop4": 0, "coop2": 1}  # rt_frame.hot_kernel (RT_HOT_*)
DEALING = {"default": 0, "global": 1, "rows": 2, "columns": 3, "blocks": 4, "row_major": 5}
ACCEL = {"auto": 0, "reference": 1, "gpu": 2, "host": 3}
ACCEL_NAMES = {v: k for k, v in ACCEL.items()}
FLAG_COUNTERS = 1
FLAG_UNPACKED_STACK = 2  # the builds scenes of more than 2^24 wide nodes run (rt_hip.h RT_FLAG_UNPACKED_STACK)
FLAG_UNPACKED_TRIS = 4   # the builds scenes of 2^26 or more triangles run (RT_FLAG_UNPACKED_TRIS)
FLAG_POOL_CURSOR = 8     # the pool kernels' cursor hand-out, as where the job lists do not fit (RT_FLAG_POOL_CURSOR)
QUERY_CHUNK = 256  # rays a wave of the query kernel takes at once (rt_query.hpp QUERY_CHUNK)


class RtError(RuntimeError):
    pass


class Outputs(ctypes.Structure):
    _fields_ = [("rgb", ctypes.c_void_p), ("hit", ctypes.c_void_p), ("t", ctypes.c_void_p),
                ("bounce_hit", ctypes.c_void_p), ("bgra", ctypes.c_void_p)]


_lib.hip()  # fail loudly at import if the HIP library is absent
_L = _lib.hip()
_L.rt_render.argtypes = [ctypes.c_void_p, P(Camera), P(Frame), P(Outputs)]
_L.rt_gather.argtypes = [P(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]
_L.rt_download_bmp.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]


def lib_md5():
    """md5 of the librt_hip.so this process loaded"""
    return _lib.lib_md5("librt_hip.so")


def device_count():
    return _L.rt_device_count()


def gather(renderers, root=0, out=None):
    """rt_gather: the last renders of several Renderers (frames or frame batches whose rows partition each
    frame) -> renderers[root]'s device frames; afterwards renderers[root].download() / download_bmp() return
    the full frame. out: a contiguous device tensor for the full frames instead (rt_gather_to), e.g. a batch
    [frames, H, W, 3] f32 or [frames, H, W] int32 (BGRA8)."""
    arr = (ctypes.c_void_p * len(renderers))(*[r._ctx.value for r in renderers])
    if out is not None:
        rc = _L.rt_gather_to(arr, len(renderers), root, ctypes.c_void_p(_gather_out(renderers[root], out)))
    else:
        rc = _L.rt_gather(arr, len(renderers), root)
    r = renderers[root]
    r._chk(rc, "rt_gather")
    W, H = r._size
    r._last = (W, H)


def _gather_out(r, out):
    """device pointer of a gather's full-frame output tensor: contiguous, on the root's device, of the root's
    last render's pixel format (float32 for rgb, int32 for BGRA8: rt_gather_to / rt_comm_gather move the bgra
    pixels when the render wrote them) and holding every frame of that render (frames x H x W x words); a
    short or mistyped tensor is refused here rather than overrun on the device"""
    import torch
    if not hasattr(r, "_size"):
        raise RtError("gather out: the root renderer has not rendered")
    W, H = r._size
    words = r._words
    want = torch.int32 if words == 1 else torch.float32
    return _ptr(out, "gather out", r._frames * W * H * words, (want,), r.device)


COMM_ID_BYTES = 128  # RT_COMM_ID_BYTES


def comm_id():
    """rt_comm_get_id: a fresh RCCL unique id (bytes) for rt_comm_init_rank; rank 0 makes it, every rank gets it"""
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    if _L.rt_comm_get_id(buf) != 0:
        raise RtError("rt_comm_get_id failed")
    return buf.raw


class Comm:
    """rt_comm: an RCCL communicator over Renderers (SURVEY §8e's framebuffer gather over xGMI).
    Comm(renderers): one process, one Renderer per device (rt_comm_init); Comm([renderer], nranks, rank, id):
    one rank of a multi-process job (rt_comm_init_rank)."""

    def __init__(self, renderers, nranks=None, rank=None, uid=None):
        self._r = list(renderers)
        self._c = ctypes.c_void_p()
        if nranks is None:
            arr = (ctypes.c_void_p * len(self._r))(*[r._ctx.value for r in self._r])
            rc = _L.rt_comm_init(arr, len(self._r), ctypes.byref(self._c))
        else:
            assert len(self._r) == 1 and uid is not None and len(uid) == COMM_ID_BYTES
            rc = _L.rt_comm_init_rank(self._r[0]._ctx, nranks, rank, ctypes.create_string_buffer(uid, COMM_ID_BYTES),
                                      ctypes.byref(self._c))
        if rc != 0:
            raise RtError(f"rt_comm_init: {rc} ({_L.rt_last_error(self._r[0]._ctx).decode()})")
        self.rank0 = 0 if rank is None else rank

    def gather(self, root=0, out=None, src=None):
        """rt_comm_gather: every rank's last render -> the root's full frames; `out` (root only): a contiguous
        device tensor [frames, H, W, 3] f32 or [frames, H, W] int32 (BGRA8), else the root Renderer's own
        buffer (its download() / download_bmp() then read the full frame). src (multi-process communicators): the
        Renderer of this rank whose last render to send (rt_comm_gather_from; default: the one it was built with)."""
        ptr = None
        here = [src] if src is not None else self._r
        if out is not None:
            ptr = ctypes.c_void_p(_gather_out(here[root - self.rank0] if 0 <= root - self.rank0 < len(here)
                                              else here[0], out))
        if src is not None:
            if all(src is not x for x in self._r):
                self._r.append(src)  # (kept alive while the communicator may still use its stream)
            rc = _L.rt_comm_gather_from(self._c, src._ctx, root, ptr)
        else:
            rc = _L.rt_comm_gather(self._c, root, ptr)
        if rc != 0:
            raise RtError(f"rt_comm_gather: {rc} ({_L.rt_comm_last_error(self._c).decode()})")
        lr = root - self.rank0
        if 0 <= lr < len(here):
            r = here[lr]
            r._last = r._size

    def set_timeout(self, seconds):
        """rt_comm_set_timeout: the deadline of every host wait on a collective (a peer that never joins turns into
        RT_E_TIMEOUT and an aborted communicator instead of a hang)"""
        if _L.rt_comm_set_timeout(self._c, float(seconds)) != 0:
            raise RtError("rt_comm_set_timeout failed")

    def relayout(self):
        """rt_comm_relayout (collective): the next gather exchanges the ranks' row sets again"""
        if _L.rt_comm_relayout(self._c) != 0:
            raise RtError("rt_comm_relayout failed")

    def wait(self):
        """rt_comm_wait: bounded wait for the last gather; raises on a timeout (the communicator is aborted)"""
        rc = _L.rt_comm_wait(self._c)
        if rc != 0:
            raise RtError(f"rt_comm_wait: {rc} ({_L.rt_comm_last_error(self._c).decode()})")

    def info(self):
        """rt_comm_get_info: gathers, descriptor exchanges (one per layout), layouts checked pixel by pixel"""
        i = _lib.CommInfo()
        if _L.rt_comm_get_info(self._c, ctypes.byref(i)) != 0:
            raise RtError("rt_comm_get_info failed")
        return {f: getattr(i, f) for f, _ in _lib.CommInfo._fields_}

    def close(self):
        if self._c:
            _L.rt_comm_destroy(self._c)
            self._c = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _ptr(x, what="", n=0, dtypes=(), device=None):
    """device pointer of a torch tensor / raw int pointer / None. A tensor must be contiguous, of one of
    `dtypes`, on `device` and hold at least n elements (the kernel writes n of them); raw pointers are the
    caller's responsibility."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    import torch
    if not isinstance(x, torch.Tensor):
        raise RtError(f"{what}: expected a torch tensor, an int pointer or None, got {type(x).__name__}")
    if not x.is_contiguous():
        raise RtError(f"{what}: tensor is not contiguous")
    if dtypes and x.dtype not in dtypes:
        raise RtError(f"{what}: dtype {x.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
    if x.numel() < n:
        raise RtError(f"{what}: {x.numel()} elements, the frame needs {n}")
    if x.device.type != "cuda" or (device is not None and x.device.index != device):
        raise RtError(f"{what}: tensor on {x.device}, expected cuda:{device}")
    return x.data_ptr()


def _rows(rows, height):
    """rows tuple (offset, stride, n[, block[, frame_shift]]) -> rt_frame fields; None = full frame"""
    if rows is None:
        return 0, 1, height, 1, 0
    r = tuple(rows)
    return r + (1, 0)[len(r) - 3:] if len(r) < 5 else r[:5]


class Renderer:
    """One rt_ctx on one device (gpu.cuh:23-26 seam, explicit instead of global)."""

    def __init__(self, device=0, counters=False, stream=None, flags=0):
        """flags: more rt_opts.flags (FLAG_UNPACKED_STACK / FLAG_UNPACKED_TRIS: the unpacked builds for any scene)"""
        self._ctx = ctypes.c_void_p()
        opts = Opts(device, (FLAG_COUNTERS if counters else 0) | flags, stream)
        rc = _L.rt_create(ctypes.byref(opts), ctypes.byref(self._ctx))
        if rc != 0:
            raise RtError(f"rt_create(device={device}) failed with status {rc}")
        self.device = device
        self.scene = None

    def _chk(self, rc, what):
        if rc != 0:
            raise RtError(f"{what}: status {rc}: {_L.rt_last_error(self._ctx).decode()}")

    def upload(self, scene, accel="auto", ploc_radius=0, collapse_node_cost=0.0):
        """load_to_gpu(): scene = prt.host.Scene with a built BVH (the reference's bvh_build output).
        accel="auto" / "gpu": the library builds the fast kernel's BVH on the GPU (PLOC, rt_build.hpp) and
        collapses it to the 8-wide layout ("host": a binned SAH on the host instead; "auto" falls back to it
        when the GPU tree is too deep for the wide walk); accel="reference": the fast kernel traverses the given
        BVH too."""
        if scene.nodes is None:
            raise RtError("upload: build the BVH first")
        tris = np.ascontiguousarray(scene.triangles)
        nodes = np.ascontiguousarray(scene.nodes)
        idx = np.ascontiguousarray(scene.tri_idx, dtype=np.int32)
        lights = np.ascontiguousarray(scene.lights)
        d = SceneDesc(tris.ctypes.data_as(P(Triangle)), len(tris), nodes.ctypes.data_as(P(BvhNode)), len(nodes),
                      idx.ctypes.data_as(P(ctypes.c_int)),
                      lights.ctypes.data_as(P(Light)) if len(lights) else None, len(lights), Vec3(*scene.amb),
                      ACCEL.get(accel, accel), ploc_radius, collapse_node_cost)
        self._chk(_L.rt_upload_scene(self._ctx, ctypes.byref(d)), "rt_upload_scene")
        self.scene = scene
        return self

    def _frame(self, width, height, rows, bounces, spp, kernel, variant, tune, waves_cap, dealing, regroup, hot_pct=0,
               hot_kernel="coop4"):
        ro, rs, nr, rb, sh = _rows(rows, height)
        if isinstance(kernel, str) and kernel in VARIANTS:
            kernel, variant = "fast", kernel
        v = VARIANTS.get(variant, variant) if variant is not None else 0
        return Frame(width, height, ro, rs, nr, bounces, spp, KERNELS.get(kernel, kernel), rb, sh, v,
                     1 if tune else 0, waves_cap, DEALING.get(dealing, dealing), regroup, hot_pct,
                     HOT_KERNELS.get(hot_kernel, hot_kernel)), nr

    def _outputs(self, nf, nr, width, bounces, rgb, hit, t, bounce_hit, bgra):
        import torch
        n = nf * nr * width
        i32 = (torch.int32,)
        return Outputs(_ptr(rgb, "rgb", 3 * n, (torch.float32,), self.device),
                       _ptr(hit, "hit", n, i32, self.device), _ptr(t, "t", n, (torch.float32,), self.device),
                       _ptr(bounce_hit, "bounce_hit", n * bounces, i32, self.device),
                       _ptr(bgra, "bgra", n, (torch.int32, getattr(torch, "uint32", torch.int32)), self.device))

    def render(self, cam, width, height, rows=None, bounces=4, spp=1, kernel="auto", rgb=None, hit=None, t=None,
               bounce_hit=None, bgra=None, variant=None, tune=False, waves_cap=0, dealing="default", regroup=0,
               hot_pct=0, hot_kernel="coop4"):
        """render_frame(): asynchronous. rows = (offset, stride, n[, block[, frame_shift]]) (rt_frame; prt.dist)
        or None for the full frame.
        rgb / hit / t / bounce_hit ([n, W, bounces] int32) / bgra ([n, W] int32: the BMP-quantised pixel in
        top-down rows, rt_outputs.bgra): optional device tensors (torch: checked for size, dtype, device and
        contiguity) or raw pointers. variant / tune / waves_cap / dealing / regroup / hot_pct / hot_kernel: the fast
        kernel's launch configuration (rt_frame; VARIANTS, DEALING, HOT_KERNELS)."""
        f, nr = self._frame(width, height, rows, bounces, spp, kernel, variant, tune, waves_cap, dealing, regroup,
                            hot_pct, hot_kernel)
        out = self._outputs(1, nr, width, bounces, rgb, hit, t, bounce_hit, bgra)
        self._chk(_L.rt_render(self._ctx, ctypes.byref(cam), ctypes.byref(f), ctypes.byref(out)), "rt_render")
        self._last = (width, nr)
        self._size = (width, height)
        self._frames = 1
        self._words = 1 if bgra is not None else 3  # the payload a gather moves (rt_hip.hip payload_of)

    def render_frames(self, cams, width, height, rows=None, bounces=4, spp=1, kernel="auto", rgb=None, hit=None,
                      t=None, bounce_hit=None, bgra=None, variant=None, tune=False, waves_cap=0, dealing="default",
                      regroup=0):
        """rt_render_frames(): a batch of len(cams) frames of one shape (one persistent launch on the fast
        kernel); outputs [n_frames, n_rows, W, ...]. Asynchronous."""
        f, nr = self._frame(width, height, rows, bounces, spp, kernel, variant, tune, waves_cap, dealing, regroup)
        out = self._outputs(len(cams), nr, width, bounces, rgb, hit, t, bounce_hit, bgra)
        arr = (Camera * len(cams))(*cams)
        self._chk(_L.rt_render_frames(self._ctx, arr, len(cams), ctypes.byref(f), ctypes.byref(out)),
                  "rt_render_frames")
        self._last = (width, nr)
        self._size = (width, height)
        self._frames = len(cams)
        self._words = 1 if bgra is not None else 3

    def sync(self):
        ms = ctypes.c_float()
        self._chk(_L.rt_sync(self._ctx, ctypes.byref(ms)), "rt_sync")
        return ms.value

    def kernel_times(self, n):
        """per-launch kernel ms of the last n renders (HIP events on the launch stream)"""
        buf = (ctypes.c_float * max(n, 1))()
        got = _L.rt_kernel_times(self._ctx, buf, n)
        if got < 0:
            self._chk(got, "rt_kernel_times")
        return [buf[i] for i in range(got)]

    def download(self, hit=False):
        """load_from_gpu(): the last frame's compact rows -> (rgb[n_rows, W, 3], hit or None)"""
        W, nr = self._last
        nf = getattr(self, "_frames", 1)
        shp = (nr, W) if nf == 1 else (nf, nr, W)
        rgb = np.zeros(shp + (3,), np.float32)
        h = np.zeros(shp, np.int32) if hit else None
        self._chk(_L.rt_download(self._ctx, rgb.ctypes.data, h.ctypes.data if hit else None), "rt_download")
        return rgb, h

    def download_bmp(self):
        """bmp_write_file's bytes of the last (full) frame, quantised on the device (rt_download_bmp)"""
        W, H = self._size
        buf = np.zeros(54 + 4 * W * H, np.uint8)
        self._chk(_L.rt_download_bmp(self._ctx, buf.ctypes.data, buf.size), "rt_download_bmp")
        return buf.tobytes()

    def scene_info(self):
        """rt_get_scene_info: what the last upload built (accel_built: "host" = host binned SAH, "gpu" = PLOC on
        the device, "reference" = the handed-over BVH), the wide BVH's size and depth, build times"""
        i = _lib.SceneInfo()
        self._chk(_L.rt_get_scene_info(self._ctx, ctypes.byref(i)), "rt_get_scene_info")
        d = {f: getattr(i, f) for f, _ in _lib.SceneInfo._fields_}
        d["accel_built"] = ACCEL_NAMES.get(d["accel_built"], d["accel_built"])
        return d

    def launch_info(self):
        """rt_get_launch_info: what the last render ran (variant name, hot tiles, cold kernel) and whether it was a
        measuring / trial frame of the default rule (`trial`) or the shape's decided configuration (`settled`);
        no synchronisation"""
        i = _lib.LaunchInfo()
        self._chk(_L.rt_get_launch_info(self._ctx, ctypes.byref(i)), "rt_get_launch_info")
        d = {f: getattr(i, f) for f, _ in _lib.LaunchInfo._fields_}
        d["variant"] = VARIANT_NAMES.get(d["variant"], d["variant"])
        d["cold_variant"] = VARIANT_NAMES.get(d["cold_variant"], d["cold_variant"])
        d["build_bits"] = sorted(k for k, v in _lib.BUILD_BITS.items() if d["build"] & v)
        return d

    def _rays(self, origins, dirs):
        """device pointers and count of a query's rays: [n, 3] float32 contiguous tensors on this device (checked
        before any launch), or raw pointers with n = origins' (an (int pointer, n) pair)"""
        import torch
        if isinstance(origins, tuple):  # raw pointers: (pointer, n); dirs a raw pointer
            po, n = origins
            if not isinstance(po, int) or not isinstance(dirs, int) or n < 0:
                raise RtError("rays: raw pointers are given as origins=(pointer, n), dirs=pointer")
            return po, dirs, int(n)
        for x, what in ((origins, "origins"), (dirs, "dirs")):
            if not isinstance(x, torch.Tensor):
                raise RtError(f"{what}: expected a torch tensor or a raw (pointer, n), got {type(x).__name__}")
            if x.dim() != 2 or x.shape[1] != 3:
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, 3]")
        n = origins.shape[0]
        if dirs.shape[0] != n:
            raise RtError(f"dirs: {dirs.shape[0]} rays, origins has {n}")
        f32 = (torch.float32,)
        return _ptr(origins, "origins", 3 * n, f32, self.device), _ptr(dirs, "dirs", 3 * n, f32, self.device), n

    def _points(self, points, max_dist2, point, tail):
        """(points pointer, max_dist2 pointer or None, n) of a nearest / nearest_tris call: points a [n, 3] float32
        contiguous tensor on this device or a raw (pointer, n), max_dist2 an optional [n] float32 tensor; the caller's
        `point` output, when a tensor, has the shape [n, *tail]. Shapes are checked before devices and dtypes."""
        import torch
        f32 = (torch.float32,)
        if isinstance(points, tuple):  # a raw pointer: (pointer, n)
            pp, n = points
            if not isinstance(pp, int) or not isinstance(n, int) or n < 0:
                raise RtError("points: a raw pointer is given as points=(pointer, n)")
        else:
            if not isinstance(points, torch.Tensor):
                raise RtError(f"points: expected a torch tensor or a raw (pointer, n), got {type(points).__name__}")
            if points.dim() != 2 or points.shape[1] != 3:
                raise RtError(f"points: shape {tuple(points.shape)}, expected [n, 3]")
            n = points.shape[0]
        if isinstance(max_dist2, torch.Tensor) and max_dist2.dim() != 1:
            raise RtError(f"max_dist2: shape {tuple(max_dist2.shape)}, expected [n]")
        if isinstance(point, torch.Tensor) and (point.dim() != 1 + len(tail) or tuple(point.shape[1:]) != tail):
            raise RtError(f"point: shape {tuple(point.shape)}, expected [n, {', '.join(map(str, tail))}]")
        if not isinstance(points, tuple):
            pp = _ptr(points, "points", 3 * n, f32, self.device)
        if max_dist2 is not None and not isinstance(max_dist2, (torch.Tensor, int)):
            raise RtError(f"max_dist2: expected a torch tensor, got {type(max_dist2).__name__}")
        return pp, _ptr(max_dist2, "max_dist2", n, f32, self.device), n

    def _info(self, struct, fn):
        """the counters a rt_get_*_info call fills, as a dict (the call synchronises and raises on an overflowed stack)"""
        i = struct()
        self._chk(getattr(_L, fn)(self._ctx, ctypes.byref(i)), fn)
        return {f: getattr(i, f) for f, _ in struct._fields_}

    def _trace(self, rays, res):
        self._chk(_L.rt_trace_rays(self._ctx, ctypes.byref(rays), ctypes.byref(res)), "rt_trace_rays")

    def trace_rays(self, origins, dirs, kernel="auto", hit=None, t=None, regroup=0):
        """rt_trace_rays(RT_QUERY_CLOSEST): the closest hit of each ray o + t d, as the reference's bvh_traverse
        finds it (bit-exact, first-found at exact ties) -> (hit [n] int32: original triangle index, -1 = miss;
        t [n] float32: the ray parameter, FLT_MAX on a miss). origins / dirs: [n, 3] float32 contiguous tensors on
        this device (dirs are not normalised), or origins=(pointer, n), dirs=pointer; hit / t: optional outputs
        (allocated when not given). Asynchronous on the renderer's stream: sync() or query_info() before the results
        are read on another stream."""
        import torch
        po, pd, n = self._rays(origins, dirs)
        dev = f"cuda:{self.device}"
        if hit is None:
            hit = torch.empty(n, dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty(n, dtype=torch.float32, device=dev)
        res = _lib.RayResults(_ptr(hit, "hit", n, (torch.int32,), self.device),
                              _ptr(t, "t", n, (torch.float32,), self.device), None)
        self._trace(_lib.Rays(po, pd, None, n, 0, KERNELS.get(kernel, kernel), regroup), res)
        return hit, t

    def occluded(self, origins, dirs, max_dist2, kernel="auto", out=None, regroup=0):
        """rt_trace_rays(RT_QUERY_OCCLUDED): out[i] = 1 when the reference's bvh_light_traverse finds a triangle
        on ray i nearer than max_dist2[i] (a squared distance, [n] float32), else 0 -> out [n] int32.
        regroup (fast kernel): the pool kernel's refill threshold in idle lanes (0: the default; 64: the lockstep
        kernel instead); the answer does not depend on it"""
        import torch
        po, pd, n = self._rays(origins, dirs)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=f"cuda:{self.device}")
        pm = _ptr(max_dist2, "max_dist2", n, (torch.float32,), self.device)
        if pm is None:
            raise RtError("max_dist2: expected a tensor or a raw pointer")
        res = _lib.RayResults(None, None, _ptr(out, "out", n, (torch.int32,), self.device))
        self._trace(_lib.Rays(po, pd, pm, n, 1, KERNELS.get(kernel, kernel), regroup), res)
        return out

    def query_info(self):
        """rt_get_query_info: the last query's counters (rays, hits, the rays each view served, strict_rays outside
        the fast walk's domain, tie_rewalks) and kernel_ms; synchronises; raises when the query overflowed a stack"""
        return self._info(_lib.QueryInfo, "rt_get_query_info")

    def shade_rays(self, origins, dirs, bounces=4, kernel="auto", regroup=0, unclamped=False, rgb=None, bgra=None,
                   hit=None, t=None, bounce_hit=None):
        """rt_shade_rays: the colour the reference's raytrace() gives each ray o + t d (shading, shadow rays, the
        reflection chain of `bounces` levels; bit-exact) -> rgb [n, 3] float32, clamped to [0, 1] like a frame's pixel
        (unclamped=True: raytrace()'s value as is). Rays as trace_rays takes them (prt.rays makes some). Optional
        outputs: bgra [n] int32 (the BMP-quantised pixel; not with unclamped), hit [n] int32 and t [n] float32 (the
        level-0 closest hit, trace_rays' answer), bounce_hit [n, bounces] int32. rgb is allocated when no output is
        given, and returned (None when other outputs were given without it). regroup (fast kernel): the shadow pool's
        refill threshold in idle lanes, 64 = the lockstep form, 0 = the library's choice; the answer does not depend
        on it. Asynchronous on the renderer's stream: sync() or shade_info() before reading on another stream."""
        import torch
        if unclamped and bgra is not None:
            raise RtError("shade_rays: unclamped has no bgra quantisation")
        po, pd, n = self._rays(origins, dirs)
        if rgb is None and bgra is None and hit is None and t is None and bounce_hit is None:
            rgb = torch.empty((n, 3), dtype=torch.float32, device=f"cuda:{self.device}")
        i32 = (torch.int32,)
        res = _lib.ShadeResults(_ptr(rgb, "rgb", 3 * n, (torch.float32,), self.device),
                                _ptr(bgra, "bgra", n, (torch.int32, getattr(torch, "uint32", torch.int32)), self.device),
                                _ptr(hit, "hit", n, i32, self.device), _ptr(t, "t", n, (torch.float32,), self.device),
                                _ptr(bounce_hit, "bounce_hit", n * bounces, i32, self.device))
        q = _lib.Shade(po, pd, n, bounces, KERNELS.get(kernel, kernel), regroup, 1 if unclamped else 0)
        self._chk(_L.rt_shade_rays(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_shade_rays")
        return rgb

    def shade_info(self):
        """rt_get_shade_info: the last shade query's counters (rays, hits, reflection, shadow, shadow_skipped as
        stats() counts a frame's; strict_paths outside the fast walks' domain; tie_rewalks) and kernel_ms;
        synchronises; raises when the query overflowed a stack"""
        return self._info(_lib.ShadeInfo, "rt_get_shade_info")

    def trace_hits(self, origins, dirs, max_hits=8, t_max=None, count_all=False, kernel="auto", tri=None, t=None,
                   count=None):
        """rt_trace_hits: the max_hits nearest hits of each ray o + t d among ALL triangles hit_triangle accepts with
        t <= t_max -- ordered by (t, original triangle index), the reference's brute-force answer whatever the BVH ->
        (tri [n, max_hits] int32, -1 in unused slots; t [n, max_hits] float32, FLT_MAX in unused slots; count [n]
        int32 = min(hits, max_hits), or every hit of the ray with count_all=True, when the walk prunes at t_max only).
        max_hits: 0..16; 0 with count_all=True is a pure counting query (tri and t come back empty). t_max: optional
        [n] float32 tensor (+inf: no bound; NaN or <= 0: no hits). Rays as trace_rays takes them; kernel="strict" tests
        every triangle (the checker), "fast" / "auto" walks the wide views with the same bits. Asynchronous on the
        renderer's stream: sync() or hits_info() before the results are read on another stream."""
        import torch
        if not isinstance(max_hits, int) or isinstance(max_hits, bool) or not 0 <= max_hits <= _lib.HITS_MAX:
            raise RtError(f"max_hits: {max_hits!r}, expected an int in 0..{_lib.HITS_MAX}")
        if max_hits == 0 and not count_all:
            raise RtError("max_hits = 0 stores nothing: it needs count_all=True")
        po, pd, n = self._rays(origins, dirs)
        f32, i32 = (torch.float32,), (torch.int32,)
        if isinstance(t_max, torch.Tensor) and t_max.dim() != 1:
            raise RtError(f"t_max: shape {tuple(t_max.shape)}, expected [n]")
        pm = _ptr(t_max, "t_max", n, f32, self.device)
        for x, what, k, dt in ((tri, "tri", n * max_hits, i32), (t, "t", n * max_hits, f32), (count, "count", n, i32)):
            _ptr(x, what, k, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, max_hits), dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty((n, max_hits), dtype=torch.float32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        res = _lib.HitResults(_ptr(tri, "tri", n * max_hits, i32, self.device) if max_hits else None,
                              _ptr(t, "t", n * max_hits, f32, self.device) if max_hits else None,
                              _ptr(count, "count", n, i32, self.device))
        q = _lib.Hits(po, pd, pm, n, max_hits, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_trace_hits(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_trace_hits")
        return tri, t, count

    def hits_info(self):
        """rt_get_hits_info: the last hits query's counters (rays, rays_hit, hits_stored, hits_counted, the rays each
        view served, exhaustive_rays tested against every triangle) and kernel_ms; synchronises; raises when the query
        overflowed a stack"""
        return self._info(_lib.HitsInfo, "rt_get_hits_info")

    def nearest(self, points, max_dist2=None, kernel="auto", tri=None, d2=None, point=None):
        """rt_nearest_points: per point the nearest triangle of the scene, the squared distance to it and the closest
        point on it -- the first triangle by (D, original triangle index), whatever the BVH (include/rt_hip.h states D
        and P) -> (tri [n] int32, -1 when nothing lies within the bound; d2 [n] float32, FLT_MAX then; point [n, 3]
        float32, the query point's own bits then). points: a [n, 3] float32 contiguous tensor on this device, or a raw
        (pointer, n).
        max_dist2: optional [n] float32 tensor of squared bounds (+inf: none; 0: points on the surface; NaN or
        negative: nothing). kernel="strict" tests every triangle (the checker), "fast" / "auto" walks the full wide view
        with the same bits. tri / d2 / point: optional outputs (allocated when not given). Asynchronous on the
        renderer's stream: sync() or nearest_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        pp, pm, n = self._points(points, max_dist2, point, (3,))
        for x, what, k, dt in ((tri, "tri", n, i32), (d2, "d2", n, f32), (point, "point", 3 * n, f32)):
            _ptr(x, what, k, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty(n, dtype=torch.int32, device=dev)
        if d2 is None:
            d2 = torch.empty(n, dtype=torch.float32, device=dev)
        if point is None:
            point = torch.empty((n, 3), dtype=torch.float32, device=dev)
        res = _lib.NearestResults(_ptr(tri, "tri", n, i32, self.device), _ptr(d2, "d2", n, f32, self.device),
                                  _ptr(point, "point", 3 * n, f32, self.device))
        q = _lib.Points(pp, pm, n, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_nearest_points(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_nearest_points")
        return tri, d2, point

    def nearest_info(self):
        """rt_get_nearest_info: the last nearest query's counters (points, found, walked_points, exhaustive_points,
        empty_points, nodes_visited, tris_tested) and kernel_ms; synchronises; raises when the query overflowed its
        stack"""
        return self._info(_lib.NearestInfo, "rt_get_nearest_info")

    def nearest_tris(self, points, k=8, max_dist2=None, count_all=False, points_out=False, kernel="auto", tri=None,
                     d2=None, count=None, point=None):
        """rt_nearest_tris: per point the k nearest triangles of the scene -- the first k by (D, original triangle
        index) among those with D <= max_dist2, nearest's own order (include/rt_hip.h) -> (tri [n, k] int32, -1 in
        unused slots; d2 [n, k] float32, FLT_MAX in unused slots; count [n] int32 = min(triangles within the bound, k),
        or every triangle within the bound with count_all=True, when the walk prunes at the bound only), plus point
        [n, k, 3] float32 (the closest point on each triangle; the query point's own bits in unused slots) with
        points_out=True or a `point` output. k: 0..16; 0 with count_all=True is a pure radius count (tri and d2 come
        back empty). With k = 1 the answer is nearest's, bit for bit. points, max_dist2 and kernel as nearest takes
        them; without a bound count_all counts every triangle of the scene, a full traversal. tri / d2 / count / point:
        optional outputs (allocated when not given). Asynchronous on the renderer's stream: sync() or
        neighbours_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.NEIGHBOURS_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.NEIGHBOURS_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        pp, pm, n = self._points(points, max_dist2, point, (k, 3))
        for x, what, m, dt in ((tri, "tri", n * k, i32), (d2, "d2", n * k, f32), (count, "count", n, i32),
                               (point, "point", 3 * n * k, f32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if d2 is None:
            d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        if point is None and points_out:
            point = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        res = _lib.NeighbourResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                                    _ptr(d2, "d2", n * k, f32, self.device) if k else None,
                                    _ptr(point, "point", 3 * n * k, f32, self.device) if k else None,
                                    _ptr(count, "count", n, i32, self.device))
        q = _lib.Neighbours(pp, pm, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_nearest_tris(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_nearest_tris")
        return (tri, d2, count) if point is None else (tri, d2, count, point)

    def neighbours_info(self):
        """rt_get_neighbours_info: the last neighbours query's counters (points, found, tris_stored, tris_counted,
        walked_points, exhaustive_points, empty_points, nodes_visited, tris_tested) and kernel_ms; synchronises; raises
        when the query overflowed its stack"""
        return self._info(_lib.NeighboursInfo, "rt_get_neighbours_info")

    def _boxes(self, lo, hi):
        """(lo pointer, hi pointer, n) of two [n, 3] float32 contiguous tensors on this device, or of raw pointers
        given as lo=(pointer, n), hi=pointer"""
        import torch
        if isinstance(lo, tuple):
            pl, n = lo
            if not isinstance(pl, int) or not isinstance(n, int) or n < 0 or not isinstance(hi, int):
                raise RtError("boxes: raw pointers are given as lo=(pointer, n), hi=pointer")
            return pl, hi, n
        for x, what in ((lo, "lo"), (hi, "hi")):
            if not isinstance(x, torch.Tensor):
                raise RtError(f"{what}: expected a torch tensor or raw pointers, got {type(x).__name__}")
            if x.dim() != 2 or x.shape[1] != 3:
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, 3]")
        n = lo.shape[0]
        if hi.shape[0] != n:
            raise RtError(f"hi: {hi.shape[0]} boxes, lo has {n}")
        f32 = (torch.float32,)
        return _ptr(lo, "lo", 3 * n, f32, self.device), _ptr(hi, "hi", 3 * n, f32, self.device), n

    def overlaps(self, lo, hi, k=8, count_all=False, kernel="auto", tri=None, count=None):
        """rt_overlap_boxes: per closed axis-aligned box [lo, hi] the triangles of the scene that touch it -- the first k
        by original triangle index of S_i = { j : T(lo, hi, triangle j) }, T the float32 triangle-box test
        include/rt_hip.h states -> (tri [n, k] int32, -1 in unused slots; count [n] int32 = min(|S_i|, k), or |S_i|
        itself with count_all=True). lo, hi: [n, 3] float32 contiguous tensors on this device (or raw pointers:
        lo=(pointer, n), hi=pointer). A box with lo == hi on some axes (a plane, a line, a point) is valid; a
        non-finite number or lo > hi on an axis gives the empty set. k: 0..16; 0 with count_all=True is a pure count
        (tri comes back empty). kernel="strict" tests every triangle (the checker), "fast" / "auto" walks the full wide
        view with the same answer. tri / count: optional outputs (allocated when not given). overlaps_csr gives every
        box's full set. Asynchronous on the renderer's stream: sync() or overlaps_info() before the results are read on
        another stream."""
        import torch
        i32 = (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.OVERLAPS_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.OVERLAPS_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        pl, ph, n = self._boxes(lo, hi)
        for x, what, m in ((tri, "tri", n * k), (count, "count", n)):
            _ptr(x, what, m, i32, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        res = _lib.OverlapResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                                  _ptr(count, "count", n, i32, self.device), None)
        q = _lib.Boxes(pl, ph, None, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_overlap_boxes(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_overlap_boxes")
        return tri, count

    def overlaps_info(self):
        """rt_get_overlaps_info: the last overlap query's counters (boxes, found, tris_stored, tris_counted,
        tris_listed, walked_boxes, exhaustive_boxes, empty_boxes, nodes_visited, tris_tested) and kernel_ms;
        synchronises; raises when the query overflowed its stack"""
        return self._info(_lib.OverlapsInfo, "rt_get_overlaps_info")

    @staticmethod
    def _spheres(centres, motions, radius, t_max):
        """the sweep queries' input checks -> (n, centre, motion and radius pointers when they were given raw, else
        None): centres, motions [n, 3] tensors with radius a float or an [n] tensor, or raw pointers given as
        centres=(pointer, n), motions=pointer, radius=pointer; t_max an [n] tensor, a raw pointer or None"""
        import torch
        if isinstance(centres, tuple):
            pc, n = centres
            if (not isinstance(pc, int) or not isinstance(n, int) or n < 0 or not isinstance(motions, int) or
                    isinstance(radius, bool) or not isinstance(radius, int)):
                raise RtError("spheres: raw pointers are given as centres=(pointer, n), motions=pointer, radius=pointer")
            pd, pr = motions, radius
        else:
            pc = pd = pr = None
            for x, what in ((centres, "centres"), (motions, "motions")):
                if not isinstance(x, torch.Tensor):
                    raise RtError(f"{what}: expected a torch tensor or raw pointers, got {type(x).__name__}")
                if x.dim() != 2 or x.shape[1] != 3:
                    raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, 3]")
            n = centres.shape[0]
            if motions.shape[0] != n:
                raise RtError(f"motions: {motions.shape[0]} spheres, centres has {n}")
            if isinstance(radius, torch.Tensor):
                if radius.dim() != 1:
                    raise RtError(f"radius: shape {tuple(radius.shape)}, expected [n]")
                if radius.shape[0] != n:
                    raise RtError(f"radius: {radius.shape[0]} spheres, centres has {n}")
            elif isinstance(radius, bool) or not isinstance(radius, (int, float)):
                raise RtError(f"radius: expected a float or a torch tensor, got {type(radius).__name__}")
        if t_max is not None and not isinstance(t_max, (torch.Tensor, int)):
            raise RtError(f"t_max: expected a torch tensor, got {type(t_max).__name__}")
        if isinstance(t_max, torch.Tensor) and t_max.dim() != 1:
            raise RtError(f"t_max: shape {tuple(t_max.shape)}, expected [n]")
        return n, pc, pd, pr

    def sweep(self, centres, motions, radius, t_max=None, kernel="fast", tri=None, t=None, point=None):
        """rt_sweep_spheres: per moving sphere -- centre c + t d at time t, radius r -- its first contact with the scene:
        the first triangle by (toi, original triangle index), whatever the BVH (include/rt_hip.h states toi) -> (tri [n]
        int32, -1 when nothing is touched within the bound; t [n] float32 = toi, FLT_MAX then; point [n, 3] float32 =
        the contact point, the centre's own bits then). The caller's normal is (c + t d) - point. centres, motions:
        [n, 3] float32 contiguous tensors on this device (or raw pointers: centres=(pointer, n), motions=pointer, with
        radius a raw pointer too); motions are not normalised, and d = 0 asks "does it touch now". radius: a float, or
        an [n] float32 tensor (r >= 0; 0 is a thin sweep). t_max: optional [n] float32 tensor of bounds on t (+inf: none;
        0: touching now; NaN or negative: nothing). kernel="strict" runs every sweep against every triangle (the
        checker), "fast" / "auto" walks the full wide view with the same bits. tri / t / point: optional outputs
        (allocated when not given). Asynchronous on the renderer's stream: sync() or sweep_info() before the results
        are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        n, pc, pd, pr = self._spheres(centres, motions, radius, t_max)
        if isinstance(point, torch.Tensor) and (point.dim() != 2 or point.shape[1] != 3):
            raise RtError(f"point: shape {tuple(point.shape)}, expected [n, 3]")
        if not isinstance(centres, tuple):
            pc = _ptr(centres, "centres", 3 * n, f32, self.device)
            pd = _ptr(motions, "motions", 3 * n, f32, self.device)
        pm = _ptr(t_max, "t_max", n, f32, self.device)
        for x, what, k, dt in ((tri, "tri", n, i32), (t, "t", n, f32), (point, "point", 3 * n, f32)):
            _ptr(x, what, k, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if not isinstance(centres, tuple):
            if not isinstance(radius, torch.Tensor):
                radius = torch.full((n,), float(radius), dtype=torch.float32, device=dev)
                torch.cuda.current_stream(self.device).synchronize()  # (the fill is torch's work, the query runs on ours)
            pr = _ptr(radius, "radius", n, f32, self.device)
        if tri is None:
            tri = torch.empty(n, dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty(n, dtype=torch.float32, device=dev)
        if point is None:
            point = torch.empty((n, 3), dtype=torch.float32, device=dev)
        res = _lib.SweepResults(_ptr(tri, "tri", n, i32, self.device), _ptr(t, "t", n, f32, self.device),
                                _ptr(point, "point", 3 * n, f32, self.device))
        q = _lib.Spheres(pc, pd, pr, pm, n, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_sweep_spheres(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_sweep_spheres")
        self._sweep_keep = radius  # (a radius tensor made here lives until the next sweep: the launch is asynchronous)
        return tri, t, point

    def sweep_info(self):
        """rt_get_sweep_info: the last sweep query's counters (spheres, found, empty_spheres, walked_spheres,
        exhaustive_spheres, nodes_visited, tris_tested) and kernel_ms; synchronises; raises when the query overflowed
        its stack"""
        return self._info(_lib.SweepInfo, "rt_get_sweep_info")

    def sweep_contacts(self, centres, motions, radius, k=8, t_max=None, count_all=False, points_out=False,
                       kernel="auto", tri=None, t=None, count=None, point=None):
        """rt_sweep_contacts: per moving sphere its k earliest contacts with the scene -- the first k by (toi, original
        triangle index) among the triangles with toi <= t_max, sweep's own set and order (include/rt_hip.h) -> (tri
        [n, k] int32, -1 in unused slots; t [n, k] float32 = each contact's toi, FLT_MAX in unused slots; count [n] int32
        = min(contacts within the bound, k), or every contact within the bound with count_all=True, when the walk prunes
        at the bound only), plus point [n, k, 3] float32 (each contact's own contact point, at the centre c + toi_j d;
        the centre's own bits in unused slots) with points_out=True or a `point` output. k: 0..16; 0 with
        count_all=True is a pure count (tri and t come back empty) -- with t_max = 1 the number of triangles the capsule
        from c to c + d touches. With k = 1 the answer is sweep's, bit for bit. centres, motions, radius, t_max and
        kernel as sweep takes them; without a bound count_all counts every triangle the sphere ever touches.
        tri / t / count / point: optional outputs (allocated when not given). Asynchronous on the renderer's stream:
        sync() or contacts_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.CONTACTS_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.CONTACTS_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        n, pc, pd, pr = self._spheres(centres, motions, radius, t_max)
        if isinstance(point, torch.Tensor) and (point.dim() != 3 or tuple(point.shape[1:]) != (k, 3)):
            raise RtError(f"point: shape {tuple(point.shape)}, expected [n, {k}, 3]")
        if not isinstance(centres, tuple):
            pc = _ptr(centres, "centres", 3 * n, f32, self.device)
            pd = _ptr(motions, "motions", 3 * n, f32, self.device)
        pm = _ptr(t_max, "t_max", n, f32, self.device)
        for x, what, m, dt in ((tri, "tri", n * k, i32), (t, "t", n * k, f32), (count, "count", n, i32),
                               (point, "point", 3 * n * k, f32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if not isinstance(centres, tuple):
            if not isinstance(radius, torch.Tensor):
                radius = torch.full((n,), float(radius), dtype=torch.float32, device=dev)
                torch.cuda.current_stream(self.device).synchronize()  # (the fill is torch's work, the query runs on ours)
            pr = _ptr(radius, "radius", n, f32, self.device)
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty((n, k), dtype=torch.float32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        if point is None and points_out:
            point = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        res = _lib.ContactResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                                  _ptr(t, "t", n * k, f32, self.device) if k else None,
                                  _ptr(point, "point", 3 * n * k, f32, self.device) if k else None,
                                  _ptr(count, "count", n, i32, self.device))
        q = _lib.SphereContacts(pc, pd, pr, pm, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_sweep_contacts(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_sweep_contacts")
        self._contacts_keep = radius  # (a radius tensor made here lives until the next query: the launch is asynchronous)
        return (tri, t, count) if point is None else (tri, t, count, point)

    def contacts_info(self):
        """rt_get_contacts_info: the last contacts query's counters (spheres, found, tris_stored, tris_counted,
        walked_spheres, exhaustive_spheres, empty_spheres, nodes_visited, tris_tested) and kernel_ms; synchronises;
        raises when the query overflowed its stack"""
        return self._info(_lib.ContactsInfo, "rt_get_contacts_info")

    def overlaps_csr(self, lo, hi, kernel="auto"):
        """every box's full S_i, in index order -> (offsets [n + 1] int32, tris [offsets[n]] int32): box i's triangles
        are tris[offsets[i]:offsets[i + 1]], ascending. Two launches of rt_overlap_boxes -- a pure count, then the list
        form into the counts' prefix sums -- and one sort that puts each segment in order (the list form states none).
        Synchronises (the total is read on the host); refuses a total of 2^31 or more. lo, hi and kernel as overlaps
        takes them."""
        import torch
        pl, ph, n = self._boxes(lo, hi)
        dev = f"cuda:{self.device}"
        kern = KERNELS.get(kernel, kernel)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        q = _lib.Boxes(pl, ph, None, n, 0, 1, kern)
        res = _lib.OverlapResults(None, _ptr(count, "count", n, (torch.int32,), self.device), None)
        self._chk(_L.rt_overlap_boxes(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_overlap_boxes")
        self.overlaps_info()  # (synchronises the renderer's stream with torch's; raises on an overflowed stack)
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(ends[-1]) if n else 0
        if total >= 2 ** 31:
            raise RtError(f"overlaps_csr: {total} entries in all, int32 offsets hold fewer than 2^31: split the boxes")
        offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        offsets[1:] = ends.to(torch.int32)
        tris = torch.empty(total, dtype=torch.int32, device=dev)
        if total == 0:
            return offsets, tris
        torch.cuda.current_stream(self.device).synchronize()  # (offsets is torch's work, the query runs on ours)
        q = _lib.Boxes(pl, ph, offsets.data_ptr(), n, 0, 1, kern)
        res = _lib.OverlapResults(None, count.data_ptr(), tris.data_ptr())
        self._chk(_L.rt_overlap_boxes(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_overlap_boxes")
        self.overlaps_info()
        n_tris = self.scene_info()["n_triangles"]
        seg = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), count.to(torch.int64))
        key, _ = torch.sort(seg * n_tris + tris.to(torch.int64))  # (segment-major, index ascending within each)
        return offsets, (key - seg * n_tris).to(torch.int32)

    def _tris(self, tris):
        """(pointer, n) of an [n, 3, 3] float32 contiguous tensor on this device, or of a raw pointer given as
        tris=(pointer, n)"""
        import torch
        if isinstance(tris, tuple):
            pt, n = tris if len(tris) == 2 else (None, None)
            if not isinstance(pt, int) or not isinstance(n, int) or isinstance(n, bool) or n < 0:
                raise RtError("tris: a raw pointer is given as tris=(pointer, n)")
            return pt, n
        if not isinstance(tris, torch.Tensor):
            raise RtError(f"tris: expected a torch tensor or a raw (pointer, n), got {type(tris).__name__}")
        if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
            raise RtError(f"tris: shape {tuple(tris.shape)}, expected [n, 3, 3]")
        n = tris.shape[0]
        return _ptr(tris, "tris", 9 * n, (torch.float32,), self.device), n

    def cuts(self, tris, k=8, count_all=False, kernel="auto", tri=None, count=None):
        """rt_cut_triangles: per caller-supplied triangle q0, q1, q2 the triangles of the scene that it crosses -- the
        first k by original triangle index of S_i = { j : X(q, triangle j) }, X the float32 triangle-triangle test
        include/rt_hip.h states (a coplanar pair and a zero-area query are no members) -> (tri [n, k] int32, -1 in
        unused slots; count [n] int32 = min(|S_i|, k), or |S_i| itself with count_all=True). tris: an [n, 3, 3]
        float32 contiguous tensor on this device (or a raw pointer: tris=(pointer, n)); a non-finite number gives the
        empty set. k: 0..16; 0 with count_all=True is a pure count (tri comes back empty). kernel="strict" tests every
        triangle (the checker), "fast" / "auto" walks the full wide view with the same answer. tri / count: optional
        outputs (allocated when not given). cuts_csr gives every query's full set and the cut segments. Asynchronous
        on the renderer's stream: sync() or cuts_info() before the results are read on another stream."""
        import torch
        i32 = (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.CUTS_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.CUTS_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        pt, n = self._tris(tris)
        for x, what, m in ((tri, "tri", n * k), (count, "count", n)):
            _ptr(x, what, m, i32, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        res = _lib.CutResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                              _ptr(count, "count", n, i32, self.device), None, None)
        q = _lib.Tris(pt, None, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_cut_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_cut_triangles")
        return tri, count

    def cuts_info(self):
        """rt_get_cuts_info: the last cut query's counters (triangles, found, stored, counted, listed, walked,
        exhaustive, empty, nodes_visited, pairs_tested) and kernel_ms; synchronises; raises when the query overflowed
        its stack"""
        return self._info(_lib.CutsInfo, "rt_get_cuts_info")

    def cuts_csr(self, tris, segments=True, kernel="auto"):
        """every query triangle's full S_i, in index order, with the cut segments -> (offsets [n + 1] int32, tri
        [offsets[n]] int32, seg [offsets[n], 2, 3] float32; seg is None with segments=False): query i crosses the
        triangles tri[offsets[i]:offsets[i + 1]], ascending, along seg[p] = (s0, s1) for the pair at p. Two launches
        of rt_cut_triangles -- a pure count, then the list form into the counts' prefix sums -- and one sort that puts
        each segment of the list in index order, the cut segments permuted alongside. Synchronises (the total is read
        on the host); refuses a total of 2^31 or more. tris and kernel as cuts takes them."""
        import torch
        pt, n = self._tris(tris)
        dev = f"cuda:{self.device}"
        kern = KERNELS.get(kernel, kernel)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        q = _lib.Tris(pt, None, n, 0, 1, kern)
        res = _lib.CutResults(None, _ptr(count, "count", n, (torch.int32,), self.device), None, None)
        self._chk(_L.rt_cut_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_cut_triangles")
        self.cuts_info()  # (synchronises the renderer's stream with torch's; raises on an overflowed stack)
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(ends[-1]) if n else 0
        if total >= 2 ** 31:
            raise RtError(f"cuts_csr: {total} entries in all, int32 offsets hold fewer than 2^31: split the triangles")
        offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        offsets[1:] = ends.to(torch.int32)
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        seg = torch.empty((total, 2, 3), dtype=torch.float32, device=dev) if segments else None
        if total == 0:
            return offsets, idx, seg
        torch.cuda.current_stream(self.device).synchronize()  # (offsets is torch's work, the query runs on ours)
        q = _lib.Tris(pt, offsets.data_ptr(), n, 0, 1, kern)
        res = _lib.CutResults(None, count.data_ptr(), idx.data_ptr(), seg.data_ptr() if segments else None)
        self._chk(_L.rt_cut_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_cut_triangles")
        self.cuts_info()
        n_tris = self.scene_info()["n_triangles"]
        row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), count.to(torch.int64))
        key, order = torch.sort(row * n_tris + idx.to(torch.int64))  # (query-major, index ascending within each)
        return offsets, (key - row * n_tris).to(torch.int32), seg[order] if segments else None

    def clearance(self, tris, max_dist2=None, kernel="auto", kind=None, tri=None, d2=None, on_query=None, on_mesh=None):
        """rt_clearance_triangles: per caller-supplied triangle q0, q1, q2 the nearest triangle of the scene, the squared
        distance to it and the two points where the pair comes closest -- the first triangle by (D, original triangle
        index), whatever the BVH (include/rt_hip.h states D: three corner, three mesh-corner and nine edge-pair
        candidates, and D = 0 where cuts' X holds) -> (tri [n] int32, -1 when nothing lies within the bound; d2 [n]
        float32, FLT_MAX then; on_query [n, 3] and on_mesh [n, 3] float32, q0's own bits then). tris: an [n, 3, 3]
        float32 contiguous tensor on this device (or a raw pointer: tris=(pointer, n)); a non-finite number gives the
        empty set. max_dist2: optional [n] float32 tensor of squared bounds (+inf: none; 0: what touches; NaN or
        negative: nothing). kind: an optional [n] int32 output that receives the winning candidate (0..2 a query
        corner, 3..5 a mesh corner, 6..14 an edge pair, 15 a crossing, -1 the empty set). kernel="strict" tests every
        triangle (the checker), "fast" / "auto" walks the full wide view with the same bits. tri / d2 / on_query /
        on_mesh: optional outputs (allocated when not given). A zero-area query is answered by the fifteen candidates
        alone. Asynchronous on the renderer's stream: sync() or clearance_info() before the results are read on
        another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        pt, n = self._tris(tris)
        if isinstance(max_dist2, torch.Tensor) and max_dist2.dim() != 1:
            raise RtError(f"max_dist2: shape {tuple(max_dist2.shape)}, expected [n]")
        if max_dist2 is not None and not isinstance(max_dist2, (torch.Tensor, int)):
            raise RtError(f"max_dist2: expected a torch tensor, got {type(max_dist2).__name__}")
        for x, what in ((on_query, "on_query"), (on_mesh, "on_mesh")):
            if isinstance(x, torch.Tensor) and (x.dim() != 2 or x.shape[1] != 3):
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, 3]")
        pm = _ptr(max_dist2, "max_dist2", n, f32, self.device)
        for x, what, m, dt in ((tri, "tri", n, i32), (d2, "d2", n, f32), (on_query, "on_query", 3 * n, f32),
                               (on_mesh, "on_mesh", 3 * n, f32), (kind, "kind", n, i32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty(n, dtype=torch.int32, device=dev)
        if d2 is None:
            d2 = torch.empty(n, dtype=torch.float32, device=dev)
        if on_query is None:
            on_query = torch.empty((n, 3), dtype=torch.float32, device=dev)
        if on_mesh is None:
            on_mesh = torch.empty((n, 3), dtype=torch.float32, device=dev)
        res = _lib.ClearanceResults(_ptr(tri, "tri", n, i32, self.device), _ptr(d2, "d2", n, f32, self.device),
                                    _ptr(on_query, "on_query", 3 * n, f32, self.device),
                                    _ptr(on_mesh, "on_mesh", 3 * n, f32, self.device),
                                    _ptr(kind, "kind", n, i32, self.device))
        q = _lib.ClearTris(pt, pm, n, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_clearance_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_clearance_triangles")
        return tri, d2, on_query, on_mesh

    def clearance_info(self):
        """rt_get_clearance_info: the last clearance query's counters (triangles, found, walked, exhaustive, empty,
        nodes_visited, pairs_gated, pairs_tested) and kernel_ms; synchronises; raises when the query overflowed its
        stack"""
        return self._info(_lib.ClearanceInfo, "rt_get_clearance_info")

    def _moving_tris(self, tris, motions, t_max):
        """the pointers of a triangle sweep's query triangles and motions and their count, checked as sweep_tris checks
        them, t_max's kind and shape included (its pointer is taken by the caller, after its own shape checks)"""
        import torch
        if isinstance(tris, tuple):
            if not isinstance(motions, int):
                raise RtError("motions: a raw pointer goes with tris=(pointer, n)")
        else:
            if not isinstance(motions, torch.Tensor):
                raise RtError(f"motions: expected a torch tensor, got {type(motions).__name__}")
            if motions.dim() != 2 or motions.shape[1] != 3:
                raise RtError(f"motions: shape {tuple(motions.shape)}, expected [n, 3]")
        pt, n = self._tris(tris)
        pd = _ptr(motions, "motions", 3 * n, (torch.float32,), self.device)
        if isinstance(t_max, torch.Tensor) and t_max.dim() != 1:
            raise RtError(f"t_max: shape {tuple(t_max.shape)}, expected [n]")
        if t_max is not None and not isinstance(t_max, (torch.Tensor, int)):
            raise RtError(f"t_max: expected a torch tensor, got {type(t_max).__name__}")
        return pt, n, pd

    def sweep_tris(self, tris, motions, t_max=None, kernel="fast", kind=None, tri=None, t=None, point=None):
        """rt_sweep_triangles: per moving triangle -- corners q + t d at time t, no rotation -- its first contact with
        the scene: the first triangle by (toi, original triangle index), whatever the BVH (include/rt_hip.h states toi:
        a box-against-box gate, cuts' X where the gate opens, then three query-corner, three mesh-corner and nine
        edge-pair candidates) -> (tri [n] int32, -1 when nothing is touched within the bound; t [n] float32 = toi,
        FLT_MAX then; point [n, 3] float32 = the contact point on the mesh triangle, q0's own bits then). tris: an
        [n, 3, 3] float32 contiguous tensor on this device (or a raw pointer: tris=(pointer, n), with motions a raw
        pointer too); motions: [n, 3] float32, not normalised, and d = 0 asks "does it touch now"; a non-finite number
        in either gives the empty set. t_max: optional [n] float32 tensor of bounds on t (+inf: none; 0: touching now;
        NaN or negative: nothing). kind: an optional [n] int32 output that receives the winning candidate (0..2 a query
        corner, 3..5 a mesh corner, 6..14 an edge pair, 15 a start in contact, -1 the empty set). kernel="strict" runs
        every query against every triangle (the checker), "fast" / "auto" walks the full wide view with the same bits.
        tri / t / point: optional outputs (allocated when not given). Asynchronous on the renderer's stream: sync() or
        trisweep_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        pt, n, pd = self._moving_tris(tris, motions, t_max)
        if isinstance(point, torch.Tensor) and (point.dim() != 2 or point.shape[1] != 3):
            raise RtError(f"point: shape {tuple(point.shape)}, expected [n, 3]")
        pm = _ptr(t_max, "t_max", n, f32, self.device)
        for x, what, m, dt in ((tri, "tri", n, i32), (t, "t", n, f32), (point, "point", 3 * n, f32),
                               (kind, "kind", n, i32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty(n, dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty(n, dtype=torch.float32, device=dev)
        if point is None:
            point = torch.empty((n, 3), dtype=torch.float32, device=dev)
        res = _lib.TrisweepResults(_ptr(tri, "tri", n, i32, self.device), _ptr(t, "t", n, f32, self.device),
                                   _ptr(point, "point", 3 * n, f32, self.device),
                                   _ptr(kind, "kind", n, i32, self.device))
        q = _lib.SweepTris(pt, pd, pm, n, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_sweep_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_sweep_triangles")
        return tri, t, point

    def trisweep_info(self):
        """rt_get_trisweep_info: the last triangle sweep query's counters (triangles, found, empty, walked, exhaustive,
        nodes_visited, pairs_gated, pairs_tested) and kernel_ms; synchronises; raises when the query overflowed its
        stack"""
        return self._info(_lib.TrisweepInfo, "rt_get_trisweep_info")

    def sweep_tri_contacts(self, tris, motions, k=8, t_max=None, count_all=False, points_out=False, kernel="auto",
                           tri=None, t=None, count=None, point=None, kind=None):
        """rt_sweep_tri_contacts: per moving triangle its k earliest contacts with the scene -- the first k by (toi,
        original triangle index) among the triangles with toi <= t_max, sweep_tris' own set and order
        (include/rt_hip.h) -> (tri [n, k] int32, -1 in unused slots; t [n, k] float32 = each contact's toi, FLT_MAX in
        unused slots; count [n] int32 = min(contacts within the bound, k), or every contact within the bound with
        count_all=True, when the walk prunes at the bound only), plus point [n, k, 3] float32 (each contact's own
        contact point on its mesh triangle; q0's own bits in unused slots) with points_out=True or a `point` output.
        kind: an optional [n, k] int32 output that receives each entry's winning candidate (0..15; -1 in unused slots).
        k: 0..16; 0 with count_all=True is a pure count (tri and t come back empty) -- with t_max = 1 the number of
        triangles the prism swept from q to q + d touches. With k = 1 the answer is sweep_tris', bit for bit. tris,
        motions, t_max and kernel as sweep_tris takes them; without a bound count_all counts every triangle the face
        ever touches. tri / t / count / point: optional outputs (allocated when not given). Asynchronous on the
        renderer's stream: sync() or tricontacts_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.TRICONTACTS_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.TRICONTACTS_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        pt, n, pd = self._moving_tris(tris, motions, t_max)
        for x, what in ((tri, "tri"), (t, "t"), (kind, "kind")):
            if isinstance(x, torch.Tensor) and (x.dim() != 2 or x.shape[1] != k):
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, k]")
        if isinstance(point, torch.Tensor) and (point.dim() != 3 or tuple(point.shape[1:]) != (k, 3)):
            raise RtError(f"point: shape {tuple(point.shape)}, expected [n, {k}, 3]")
        pm = _ptr(t_max, "t_max", n, f32, self.device)
        for x, what, m, dt in ((tri, "tri", n * k, i32), (t, "t", n * k, f32), (count, "count", n, i32),
                               (point, "point", 3 * n * k, f32), (kind, "kind", n * k, i32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if t is None:
            t = torch.empty((n, k), dtype=torch.float32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        if point is None and points_out:
            point = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        res = _lib.TricontactResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                                     _ptr(t, "t", n * k, f32, self.device) if k else None,
                                     _ptr(point, "point", 3 * n * k, f32, self.device) if k else None,
                                     _ptr(kind, "kind", n * k, i32, self.device) if k else None,
                                     _ptr(count, "count", n, i32, self.device))
        q = _lib.TriContacts(pt, pd, pm, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_sweep_tri_contacts(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_sweep_tri_contacts")
        return (tri, t, count) if point is None else (tri, t, count, point)

    def tricontacts_info(self):
        """rt_get_tricontacts_info: the last triangle contact query's counters (triangles, found, stored, counted,
        walked, exhaustive, empty, nodes_visited, pairs_gated, pairs_tested) and kernel_ms; synchronises; raises when
        the query overflowed its stack"""
        return self._info(_lib.TricontactsInfo, "rt_get_tricontacts_info")

    def _max_dist2(self, max_dist2, n):
        """the pointer of an optional [n] float32 tensor of squared bounds, checked as clearance checks it"""
        import torch
        if isinstance(max_dist2, torch.Tensor) and max_dist2.dim() != 1:
            raise RtError(f"max_dist2: shape {tuple(max_dist2.shape)}, expected [n]")
        if max_dist2 is not None and not isinstance(max_dist2, (torch.Tensor, int)):
            raise RtError(f"max_dist2: expected a torch tensor, got {type(max_dist2).__name__}")
        return _ptr(max_dist2, "max_dist2", n, (torch.float32,), self.device)

    def proximity(self, tris, k=8, max_dist2=None, count_all=False, pairs_out=False, kernel="auto", tri=None, d2=None,
                  count=None, on_query=None, on_mesh=None, kind=None):
        """rt_proximity_triangles: per caller-supplied triangle q0, q1, q2 the k nearest triangles of the scene -- the
        first k by (D, original triangle index) among those with D <= max_dist2, clearance's own D and order
        (include/rt_hip.h) -> (tri [n, k] int32, -1 in unused slots; d2 [n, k] float32, FLT_MAX in unused slots; count
        [n] int32 = min(triangles within the bound, k), or every triangle within the bound with count_all=True, when
        the walk prunes at the bound only), plus on_query and on_mesh [n, k, 3] float32 (the two points where each pair
        comes closest; q0's own bits in unused slots) with pairs_out=True or either output given. kind: an optional
        [n, k] int32 output that receives each entry's winning candidate (0..15; -1 in unused slots). k: 0..16; 0 with
        count_all=True is a pure count of the triangles within the margin (tri and d2 come back empty). With k = 1 the
        answer is clearance's, bit for bit. tris, max_dist2 and kernel as clearance takes them; without a bound
        count_all counts every triangle of the scene, a full traversal. tri / d2 / count / on_query / on_mesh: optional
        outputs (allocated when not given). proximity_csr gives every query's full set within a bound. Asynchronous on
        the renderer's stream: sync() or proximity_info() before the results are read on another stream."""
        import torch
        f32, i32 = (torch.float32,), (torch.int32,)
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k <= _lib.PROXIMITY_MAX:
            raise RtError(f"k: {k!r}, expected an int in 0..{_lib.PROXIMITY_MAX}")
        if k == 0 and not count_all:
            raise RtError("k = 0 stores nothing: it needs count_all=True")
        pt, n = self._tris(tris)
        for x, what in ((tri, "tri"), (d2, "d2"), (kind, "kind")):
            if isinstance(x, torch.Tensor) and (x.dim() != 2 or x.shape[1] != k):
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, k]")
        for x, what in ((on_query, "on_query"), (on_mesh, "on_mesh")):
            if isinstance(x, torch.Tensor) and (x.dim() != 3 or tuple(x.shape[1:]) != (k, 3)):
                raise RtError(f"{what}: shape {tuple(x.shape)}, expected [n, k, 3]")
        pm = self._max_dist2(max_dist2, n)
        for x, what, m, dt in ((tri, "tri", n * k, i32), (d2, "d2", n * k, f32), (count, "count", n, i32),
                               (on_query, "on_query", 3 * n * k, f32), (on_mesh, "on_mesh", 3 * n * k, f32),
                               (kind, "kind", n * k, i32)):
            _ptr(x, what, m, dt, self.device)  # (the caller's outputs are checked before anything is allocated)
        dev = f"cuda:{self.device}"
        if tri is None:
            tri = torch.empty((n, k), dtype=torch.int32, device=dev)
        if d2 is None:
            d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        if count is None:
            count = torch.empty(n, dtype=torch.int32, device=dev)
        pairs = pairs_out or on_query is not None or on_mesh is not None
        if pairs and on_query is None:
            on_query = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        if pairs and on_mesh is None:
            on_mesh = torch.empty((n, k, 3), dtype=torch.float32, device=dev)
        res = _lib.ProximityResults(_ptr(tri, "tri", n * k, i32, self.device) if k else None,
                                    _ptr(d2, "d2", n * k, f32, self.device) if k else None,
                                    _ptr(on_query, "on_query", 3 * n * k, f32, self.device) if k else None,
                                    _ptr(on_mesh, "on_mesh", 3 * n * k, f32, self.device) if k else None,
                                    _ptr(kind, "kind", n * k, i32, self.device) if k else None,
                                    _ptr(count, "count", n, i32, self.device), None, None, None, None)
        q = _lib.ProxTris(pt, pm, None, n, k, 1 if count_all else 0, KERNELS.get(kernel, kernel))
        self._chk(_L.rt_proximity_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_proximity_triangles")
        return (tri, d2, count, on_query, on_mesh) if pairs else (tri, d2, count)

    def proximity_info(self):
        """rt_get_proximity_info: the last proximity query's counters (triangles, found, stored, counted, listed,
        walked, exhaustive, empty, nodes_visited, pairs_gated, pairs_tested) and kernel_ms; synchronises; raises when
        the query overflowed its stack"""
        return self._info(_lib.ProximityInfo, "rt_get_proximity_info")

    def proximity_csr(self, tris, max_dist2, pairs=True, kernel="auto"):
        """every query triangle's full S_i within its bound, in (D, index) order, with the closest points ->
        (offsets [n + 1] int32, tri [offsets[n]] int32, d2 [offsets[n]] float32, pair [offsets[n], 2, 3] float32; pair
        is None with pairs=False): the scene's triangles tri[offsets[i]:offsets[i + 1]] lie within max_dist2[i] of
        query i, nearest first, at d2[p], the pair at p coming closest at pair[p] = (on the query, on the mesh
        triangle). Two launches of rt_proximity_triangles -- a pure count, then the list form into the counts' prefix
        sums -- and two sorts that put each segment of the list in (D, index) order, the other arrays permuted
        alongside. max_dist2: an [n] float32 tensor of squared bounds, as proximity takes it (without one every query
        lists the whole scene). Synchronises (the total is read on the host); refuses a total of 2^31 or more. tris
        and kernel as proximity takes them."""
        import torch
        pt, n = self._tris(tris)
        pm = self._max_dist2(max_dist2, n)
        dev = f"cuda:{self.device}"
        kern = KERNELS.get(kernel, kernel)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        none = (None,) * 5
        q = _lib.ProxTris(pt, pm, None, n, 0, 1, kern)
        res = _lib.ProximityResults(*none, _ptr(count, "count", n, (torch.int32,), self.device), None, None, None, None)
        self._chk(_L.rt_proximity_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_proximity_triangles")
        self.proximity_info()  # (synchronises the renderer's stream with torch's; raises on an overflowed stack)
        ends = torch.cumsum(count, 0, dtype=torch.int64)
        total = int(ends[-1]) if n else 0
        if total >= 2 ** 31:
            raise RtError(f"proximity_csr: {total} entries in all, int32 offsets hold fewer than 2^31: split the "
                          "triangles or lower the bounds")
        offsets = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        offsets[1:] = ends.to(torch.int32)
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        d2 = torch.empty(total, dtype=torch.float32, device=dev)
        pair = torch.empty((total, 2, 3), dtype=torch.float32, device=dev) if pairs else None
        if total == 0:
            return offsets, idx, d2, pair
        torch.cuda.current_stream(self.device).synchronize()  # (offsets is torch's work, the query runs on ours)
        q = _lib.ProxTris(pt, pm, offsets.data_ptr(), n, 0, 1, kern)
        res = _lib.ProximityResults(*none, count.data_ptr(), idx.data_ptr(), d2.data_ptr(),
                                    pair.data_ptr() if pairs else None, None)
        self._chk(_L.rt_proximity_triangles(self._ctx, ctypes.byref(q), ctypes.byref(res)), "rt_proximity_triangles")
        self.proximity_info()
        # (row, D, index) does not fit one int64: by D_bits << 32 | index (D >= +0: its bits order as it does), then
        # stably by row
        row = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), count.to(torch.int64))
        key = (d2.view(torch.int32).to(torch.int64) << 32) | idx.to(torch.int64)
        by_key = torch.argsort(key)
        order = by_key[torch.argsort(row[by_key], stable=True)]
        return offsets, idx[order], d2[order], pair[order] if pairs else None

    def update_vertices(self, coords):
        """rt_update_vertices: every view of the uploaded scene refitted on the device to new triangle coordinates --
        coords: a contiguous float32 tensor [n_triangles, 3, 3] on this device (the new triangle_t.coords, original
        order), e.g. a physics step's output. Afterwards every render and query gives the bits a fresh upload of the
        moved scene (same materials, same reference tree with regrown boxes) gives. Read in stream order on the
        renderer's stream; a non-finite coordinate or another triangle count is refused and changes nothing."""
        import torch
        if not isinstance(coords, torch.Tensor):
            raise RtError(f"coords: expected a torch tensor, got {type(coords).__name__}")
        if coords.dim() != 3 or tuple(coords.shape[1:]) != (3, 3):
            raise RtError(f"coords: shape {tuple(coords.shape)}, expected [n, 3, 3]")
        n = coords.shape[0]
        u = _lib.VertexUpdate(_ptr(coords, "coords", 9 * n, (torch.float32,), self.device), n)
        self._chk(_L.rt_update_vertices(self._ctx, ctypes.byref(u)), "rt_update_vertices")

    def update_info(self):
        """rt_get_update_info: what the last update_vertices did (views refitted / rebuilt, the triangles that joined
        the unit and the primary view, the new scene magnitude, the full view's area_ratio against its build) and
        update_ms; synchronises"""
        return self._info(_lib.UpdateInfo, "rt_get_update_info")

    def rebuild_views(self, coords, mode="auto"):
        """rt_rebuild_views: update_vertices(coords), then new topologies for the fast walk's wide views (full, unit,
        primary) built over those coordinates -- after large motion, when update_info()["area_ratio"] has grown. The
        reference tree stays, so every render and query returns the bits it returns after update_vertices(coords).
        mode: "device" (PLOC and the greedy collapse on the GPU; GPU-built scenes only), "host" (the upload's own build
        over downloaded coordinates) or "auto"."""
        import torch
        if not isinstance(coords, torch.Tensor):
            raise RtError(f"coords: expected a torch tensor, got {type(coords).__name__}")
        if coords.dim() != 3 or tuple(coords.shape[1:]) != (3, 3):
            raise RtError(f"coords: shape {tuple(coords.shape)}, expected [n, 3, 3]")
        if mode not in _lib.REBUILD_MODES:
            raise RtError(f"mode: {mode!r}, expected one of {sorted(_lib.REBUILD_MODES)}")
        n = coords.shape[0]
        u = _lib.ViewRebuild(_ptr(coords, "coords", 9 * n, (torch.float32,), self.device), n, _lib.REBUILD_MODES[mode])
        self._chk(_L.rt_rebuild_views(self._ctx, ctypes.byref(u)), "rt_rebuild_views")

    def rebuild_info(self):
        """rt_get_rebuild_info: what the last rebuild_views did (mode_used, fell_back, views_built, nodes / depth per
        view, the full view's area_before / area_after, rebuild_ms, host_ms and the stages' times); synchronises"""
        i = _lib.RebuildInfo()
        self._chk(_L.rt_get_rebuild_info(self._ctx, ctypes.byref(i)), "rt_get_rebuild_info")
        d = {f: getattr(i, f) for f, _ in _lib.RebuildInfo._fields_}
        d["nodes"], d["depth"] = list(i.nodes), list(i.depth)
        d["mode_used"] = {v: k for k, v in _lib.REBUILD_MODES.items()}[i.mode_used]
        return d

    def _debug_build_tree(self, view="full"):
        """test-only (rt_debug_read_build_tree): the binary tree the last device rebuild collapsed for a view ->
        (left, right, leaf_tri, root): nodes 0 .. n - 1 are leaves, leaf k holding scene triangle leaf_tri[k]; node
        n + j has the children left[j] and right[j]; or None without such a tree; synchronises"""
        v = {"full": 0, "unit": 1, "primary": 2}[view]
        root = ctypes.c_int()
        n = _L.rt_debug_read_build_tree(self._ctx, v, None, None, None, 0, ctypes.byref(root))
        if n < 0:
            self._chk(n, "rt_debug_read_build_tree")
        if n == 0:
            return None
        left, right = np.zeros(max(n - 1, 1), np.int32), np.zeros(max(n - 1, 1), np.int32)
        leaf = np.zeros(n, np.int32)
        got = _L.rt_debug_read_build_tree(self._ctx, v, left.ctypes.data, right.ctypes.data, leaf.ctypes.data, n,
                                          ctypes.byref(root))
        if got < 0:
            self._chk(got, "rt_debug_read_build_tree")
        return left[:n - 1], right[:n - 1], leaf, root.value

    def update_lights(self, lights):
        """rt_update_lights: new positions / colours for the uploaded lights (a LIGHT_DTYPE array of the same length)"""
        from .host import LIGHT_DTYPE
        lights = np.ascontiguousarray(lights, dtype=LIGHT_DTYPE)
        self._chk(_L.rt_update_lights(self._ctx, lights.ctypes.data_as(P(Light)) if len(lights) else None, len(lights)),
                  "rt_update_lights")

    def _debug_wide(self, view="full"):
        """test-only (rt_debug_read_wide): a wide view's node words [n, 20] uint32 and its position -> original
        triangle map as they stand on the device, or (None, None) without that view; synchronises"""
        v = {"full": 0, "unit": 1, "primary": 2}[view]
        n = _L.rt_debug_read_wide(self._ctx, v, None, 0, None, 0)
        if n < 0:
            self._chk(n, "rt_debug_read_wide")
        if n == 0:
            return None, None
        info = self.scene_info()
        nt = {0: info["n_triangles"], 1: info["unit_triangles"], 2: info["primary_triangles"]}[v]
        words = np.zeros((n, 20), np.uint32)
        orig = np.zeros(nt, np.int32)
        got = _L.rt_debug_read_wide(self._ctx, v, words.ctypes.data, n, orig.ctypes.data, nt)
        if got < 0:
            self._chk(got, "rt_debug_read_wide")
        return words, orig

    def stats(self):
        s = Stats()
        self._chk(_L.rt_get_stats(self._ctx, ctypes.byref(s)), "rt_get_stats")
        d = {f: getattr(s, f) for f in _lib.STAT_FIELDS}
        d["rays"] = d["primary"] + d["reflection"] + d["shadow"]
        # wave steps [kind: closest, shadow][level 0, 1, 2, 3+][active lanes 1-16, 17-32, 33-48, 49-64]
        h = list(s.steps_hist)
        d["steps_hist"] = [[h[16 * k + 4 * l:16 * k + 4 * l + 4] for l in range(4)] for k in range(2)]
        return d

    def close(self):
        if self._ctx:
            _L.rt_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
