"""Host-side Python mirror of the two Xmipp programs' inner interfaces.

Names follow the reference (ProgRecFourierAccel / ProgAngularProjectionMatching members);
every method is a thin call into libxmipp_hip.so.  torch provides device memory (tensors),
the stream and torch.distributed -- plumbing only.
"""
import ctypes as C
import weakref

import numpy as np

from ._lib import AsaParams, AsaRow, FazParams, FazRow, Ca2Params, Ca2Row, CtfParams, RfParams, XhError, check, lib


def _torch():
    import torch
    return torch


def search5d_offsets(search5d_shift, search5d_step=2):
    """Translations of the 5-D search in the reference's order (APM:321-348)."""
    if search5d_step == 0:
        search5d_step = 1
    fin = search5d_shift + search5d_shift % search5d_step
    xs, ys = [], []
    for x in range(-fin, fin + 1, search5d_step):
        for y in range(-fin, fin + 1, search5d_step):
            if x * x + y * y <= search5d_shift * search5d_shift:
                xs.append(x)
                ys.append(y)
    return np.asarray(xs, np.int32), np.asarray(ys, np.int32)


def shard_range(n, rank, world):
    """Contiguous particle range of `rank` ([g*N/G, (g+1)*N/G))."""
    return (rank * n) // world, ((rank + 1) * n) // world


class Context:
    """xh_ctx bound to torch's current stream on `device`."""

    def __init__(self, device=0):
        torch = _torch()
        L = lib()
        if not torch.cuda.is_available():
            raise XhError("no HIP device visible to torch; xmipp3_amd has no CPU fallback")
        self.device = int(device)
        torch.cuda.set_device(self.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        h = C.c_void_p()
        check(L.xh_ctx_create(self.device, C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.torch_device = torch.device("cuda", self.device)
        self._children = weakref.WeakSet()   # handles must be destroyed before their context

    def sync(self):
        check(lib().xh_ctx_sync(self.h))

    def close(self):
        if getattr(self, "h", None):
            for c in list(self._children):
                c.close()
            lib().xh_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # HIP-event timer on the library stream (bench.py roofline)
    def timer(self):
        return _Timer(self)


class _Timer:
    def __init__(self, ctx):
        self.ctx = ctx
        self.t = C.c_void_p()
        check(lib().xh_timer_create(ctx.h, C.byref(self.t)))

    def start(self):
        check(lib().xh_timer_start(self.ctx.h, self.t))

    def stop(self):
        check(lib().xh_timer_stop(self.ctx.h, self.t))

    def elapsed_ms(self):
        ms = C.c_float(0)
        check(lib().xh_timer_elapsed_ms(self.ctx.h, self.t, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if getattr(self.ctx, "h", None):
                lib().xh_timer_destroy(self.ctx.h, self.t)
        except Exception:
            pass


class _Handle:
    """A library handle made on a Context: destroyed by close() or when collected, and by its context's close() before the context
    goes. Subclasses name their xh_*_destroy in _destroy."""

    _destroy = None

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        ctx._children.add(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                getattr(lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _StageTimes:
    """set_timing / stage_ms of a handle whose entry points are xh_<_PREFIX>_set_timing and xh_<_PREFIX>_stage_ms; STAGES names what
    the second fills, in order."""

    _PREFIX = None
    STAGES = ()

    def set_timing(self, on=True):
        """runs record their stages (the benchmark's switch)"""
        check(getattr(lib(), f"xh_{self._PREFIX}_set_timing")(self.h, int(bool(on))))

    def stage_ms(self):
        """milliseconds per stage of the timed runs, a dict in the order of STAGES"""
        ms = np.zeros(len(self.STAGES))
        check(getattr(lib(), f"xh_{self._PREFIX}_stage_ms")(self.h, _np_ptr(ms)))
        return dict(zip(self.STAGES, ms))


class _VolumeHandle(_Handle):
    """A handle on one [Z, Y, X] box, made by xh_<_PREFIX>_create(ctx, Z, Y, X, *args, &h): the shape, new volumes of it, and the check
    every tensor passes before its pointer reaches the library."""

    _PREFIX = None
    _WHAT = "volume"

    def __init__(self, ctx, shape, *args):
        self.ctx = ctx
        self.shape = tuple(int(s) for s in shape)
        assert len(self.shape) == 3
        h = C.c_void_p()
        check(getattr(lib(), f"xh_{self._PREFIX}_create")(ctx.h, *self.shape, *args, C.byref(h)))
        super().__init__(ctx, h)

    def _vol(self, t, what=None, dtype=None, shape=None):
        dtype, shape = dtype or _torch().float64, shape or self.shape
        name, what = type(self).__name__, what or self._WHAT
        if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
            raise XhError(f"{name}: the {what} must be a contiguous {str(dtype).split('.')[-1]} cuda tensor")
        if tuple(t.shape) != shape:
            raise XhError(f"{name}: the {what} has shape {tuple(t.shape)}, the handle {shape}")
        return t

    def _new(self):
        return _torch().empty(self.shape, dtype=_torch().float64, device="cuda")


def _ptr(t, dtype=None):
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous()):
        raise XhError("device arguments must be contiguous cuda tensors")
    if dtype is not None and t.dtype != dtype:
        raise XhError(f"expected a {dtype} tensor, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def ctf_params(**kw):
    p = CtfParams()
    lib().xh_ctf_defaults(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, float(v))
    return p


class RecFourier(_Handle):
    """Device side of ProgRecFourierAccel (reconstruction/reconstruct_fourier_accel.cpp)."""

    _destroy = "xh_rf_destroy"

    def __init__(self, ctx, imgSize, padding_proj=2.0, padding_vol=2.0, max_resolution=0.5,
                 blob_radius=1.9, blob_order=0, blob_alpha=15.0, fast=False, phase_flipped=False,
                 min_ctf=0.01, sampling=1.0):
        torch = _torch()
        self.ctx = ctx
        p = RfParams(int(imgSize), padding_proj, padding_vol, max_resolution, blob_radius,
                     int(blob_order), blob_alpha, int(fast), int(phase_flipped), min_ctf, sampling)
        h = C.c_void_p()
        check(lib().xh_rf_create(ctx.h, C.byref(p), C.byref(h)))
        super().__init__(ctx, h)
        P, mv, sx, sy = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().xh_rf_sizes(h, C.byref(P), C.byref(mv), C.byref(sx), C.byref(sy)))
        self.D, self.P, self.mv, self.sizeX, self.sizeY = int(imgSize), P.value, mv.value, sx.value, sy.value
        # temp spaces are a torch tensor so that torch.distributed can all-reduce them in place
        self.temp = torch.zeros(lib().xh_rf_temp_floats(h), dtype=torch.float32, device=ctx.torch_device)
        check(lib().xh_rf_attach_temp(h, _ptr(self.temp)))
        self.cropped = False

    def set_option(self, name, value):
        check(lib().xh_rf_set_option(self.h, name.encode(), float(value)))

    def tables(self):
        bt = np.empty(10000, np.float32)
        fbt = np.empty(10000, np.float64)
        a, b = C.c_float(), C.c_float()
        check(lib().xh_rf_tables(self.h, _np_ptr(bt), _np_ptr(fbt), C.byref(a), C.byref(b)))
        return bt, fbt, a.value, b.value

    def reset(self):
        check(lib().xh_rf_reset(self.h))
        self.cropped = False

    def shift_images(self, imgs, shifts, flips=None, coefs=None):
        """Image::readApplyGeo(only_apply_shifts): shifts [n,2] = (shiftX, shiftY) on the host. coefs: device pointer
        (int) to the fp32 B-spline coefficients of imgs when the caller has them (ProjectionMatcher.last_coefficients)."""
        torch = _torch()
        n = imgs.shape[0]
        if isinstance(shifts, tuple) and torch.is_tensor(shifts[0]) and shifts[0].is_cuda:
            # (shiftX, shiftY) float64 tensors as ProjectionMatcher.translate returns them; flips: a uint8 tensor
            out = torch.empty_like(imgs)
            check(lib().xh_rf_shift_images_dev(self.h, _ptr(imgs, torch.float32), C.c_void_p(coefs) if coefs else None,
                                               _ptr(shifts[0], torch.float64), _ptr(shifts[1], torch.float64),
                                               _ptr(flips, torch.uint8), n, _ptr(out)))
            return out
        sh = np.ascontiguousarray(shifts, np.float32).reshape(n, 2)
        fl = None if flips is None else np.ascontiguousarray(flips, np.uint8).reshape(n)
        out = torch.empty_like(imgs)
        check(lib().xh_rf_shift_images_coefs(self.h, _ptr(imgs, torch.float32), C.c_void_p(coefs) if coefs else None,
                                             _np_ptr(sh), _np_ptr(fl), n, _ptr(out)))
        return out

    def prepare_images(self, imgs, out=None):
        """imgs: cuda float32 [n,D,D] -> [n, mv, mv/2, 2] float32 (centred half spectra)."""
        torch = _torch()
        assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.is_contiguous()
        n = imgs.shape[0]
        if out is None:
            out = torch.empty((n, self.sizeY, self.sizeX, 2), dtype=torch.float32, device=imgs.device)
        check(lib().xh_rf_prepare_images(self.h, _ptr(imgs), n, _ptr(out)))
        return out

    @staticmethod
    def ctf_param_array(ctfs):
        """Pack a list of CtfParams once (reusable across calls)."""
        return (CtfParams * len(ctfs))(*ctfs)

    def ctf_arrays(self, ctfs):
        torch = _torch()
        n = len(ctfs)
        arr = ctfs if isinstance(ctfs, C.Array) else (CtfParams * n)(*ctfs)
        c = torch.empty((n, self.sizeY, self.sizeX), dtype=torch.float32, device=self.ctx.torch_device)
        m = torch.empty_like(c)
        check(lib().xh_rf_ctf_arrays(self.h, arr, n, _ptr(c), _ptr(m)))
        return c, m

    def insert(self, fft, angles, weights=None, ctf=None, modulator=None, sym=None):
        """angles: [n,3] (rot,tilt,psi) degrees on the host."""
        n = fft.shape[0]
        ang = np.ascontiguousarray(angles, np.float64).reshape(n, 3)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        s = None if sym is None else np.ascontiguousarray(sym, np.float64).reshape(-1, 9)
        f32 = _torch().float32
        check(lib().xh_rf_insert(self.h, _ptr(fft, f32), _ptr(ctf, f32), _ptr(modulator, f32), _np_ptr(ang), _np_ptr(w), n,
                                 _np_ptr(s), 0 if s is None else s.shape[0]))

    def insert_images(self, imgs, angles, ctf_array=None, weights=None, sym=None):
        """Shifted images [n,D,D] + CTF parameters (ctf_param_array) + orientations -> temp spaces in one call
        (xh_rf_insert_images: CTF planes, FFT and insertion on scratch owned by the handle)."""
        n = imgs.shape[0]
        torch = _torch()
        s = None if sym is None else np.ascontiguousarray(sym, np.float64).reshape(-1, 9)
        if torch.is_tensor(angles) and angles.is_cuda:
            # orientations (float64 [n,3]) and weights (float32 [n]) that never left the device
            assert angles.shape == (n, 3) and angles.is_contiguous()
            check(lib().xh_rf_insert_images_dev(self.h, _ptr(imgs, torch.float32), ctf_array, _ptr(angles, torch.float64),
                                                _ptr(weights, torch.float32), n, _np_ptr(s), 0 if s is None else s.shape[0]))
            return
        ang = np.ascontiguousarray(angles, np.float64).reshape(n, 3)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        check(lib().xh_rf_insert_images(self.h, _ptr(imgs, _torch().float32), ctf_array, _np_ptr(ang), _np_ptr(w), n,
                                        _np_ptr(s), 0 if s is None else s.shape[0]))

    def insert_matrices(self, fft, ainv, weights=None, ctf=None, modulator=None, sym=None):
        n = fft.shape[0]
        a = np.ascontiguousarray(ainv, np.float64).reshape(n, 9)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        s = None if sym is None else np.ascontiguousarray(sym, np.float64).reshape(-1, 9)
        f32 = _torch().float32
        check(lib().xh_rf_insert_matrices(self.h, _ptr(fft, f32), _ptr(ctf, f32), _ptr(modulator, f32), _np_ptr(a), _np_ptr(w),
                                          n, _np_ptr(s), 0 if s is None else s.shape[0]))

    def kernel_ms(self, reset=True):
        """(total ms, launches) of the gridding kernel since the last reset (HIP events on the stream)."""
        ms, n = C.c_double(), C.c_int64()
        check(lib().xh_rf_kernel_ms(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def temp_spaces(self):
        """(volume [mv+1,mv+1,nx,2], weights [mv+1,mv+1,nx]) views of the temp tensor."""
        d = self.mv + 1
        nx = (self.mv // 2 + 1) if self.cropped else d
        tot = d * d * nx
        return self.temp[:2 * tot].view(d, d, nx, 2), self.temp[2 * tot:3 * tot].view(d, d, nx)

    def mirror_and_crop(self):
        check(lib().xh_rf_mirror_and_crop(self.h))
        self.cropped = True

    def cropped_view(self):
        """Flat view [volume | weights] of the cropped spaces: the all-reduce payload."""
        assert self.cropped
        return self.temp[:lib().xh_rf_cropped_floats(self.h)]

    def export_cropped(self):
        """Copy of the cropped spaces (a torch tensor on the handle's device); finish() consumes the
        originals, so this is how a half-set is kept for the later sum (RF:991-1045)."""
        torch = _torch()
        out = torch.empty(lib().xh_rf_cropped_floats(self.h), dtype=torch.float32, device=self.ctx.torch_device)
        check(lib().xh_rf_cropped_export(self.h, _ptr(out)))
        return out

    def import_cropped(self, buf, add=False):
        assert buf.dtype == _torch().float32 and buf.numel() == lib().xh_rf_cropped_floats(self.h)
        check(lib().xh_rf_cropped_import(self.h, _ptr(buf), 1 if add else 0))
        self.cropped = True

    def finish(self, reuse=False):
        """The finaliser; returns the D^3 volume as a numpy float64 array in page-locked memory (134 MB at D=256; from pageable
        memory the copy is the longest part of the finaliser).  Page-locking takes 25-30 ms, three times the finaliser's kernels:
        a caller that is done with the previous result before it asks for the next one says reuse=True and gets the SAME buffer
        again (its previous contents are overwritten); by default every call returns a fresh array."""
        torch = _torch()
        out = getattr(self, "_fin_out", None) if reuse else None
        if out is None:
            try:
                pin = torch.empty((self.D, self.D, self.D), dtype=torch.float64, pin_memory=True)
                out = pin.numpy()
            except RuntimeError:
                out = np.empty((self.D, self.D, self.D), np.float64)
            if reuse:
                self._fin_out = out
        check(lib().xh_rf_finish(self.h, _np_ptr(out)))
        return out


class RecFourier2(_Handle):
    """Device side of ProgRecFourier (reconstruction/reconstruct_fourier.cpp), the double-precision program behind the name
    xmipp_reconstruct_fourier. Keeps what it inserted so that finish() can replay it for --iter > 1 (correctWeight)."""

    _destroy = "xh_rf2_destroy"

    def __init__(self, ctx, imgSize, padding_proj=2.0, padding_vol=2.0, max_resolution=0.5, blob_radius=1.9, blob_order=0, blob_alpha=15.0,
                 niter_weight=1, phase_flipped=False, min_ctf=0.01, sampling=1.0):
        self.ctx, self.D, self.niter = ctx, int(imgSize), int(niter_weight)
        p = RfParams(self.D, padding_proj, padding_vol, max_resolution, blob_radius, int(blob_order), blob_alpha, 0, int(phase_flipped), min_ctf, sampling)
        h = C.c_void_p()
        check(lib().xh_rf2_create(ctx.h, C.byref(p), self.niter, C.byref(h)))
        super().__init__(ctx, h)
        self._calls = []

    def _insert(self, imgs, ctfs, ang, w, s, reprocess):
        n = ang.shape[0]
        arr = None if ctfs is None else (ctfs if isinstance(ctfs, C.Array) else (CtfParams * n)(*ctfs))
        check(lib().xh_rf2_insert(self.h, _ptr(imgs), arr, _np_ptr(ang), _np_ptr(w), n, _np_ptr(s), 0 if s is None else s.shape[0], int(reprocess)))

    def insert(self, imgs, angles, weights=None, sym=None, ctfs=None):
        torch = _torch()
        assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.is_contiguous()
        ang = np.ascontiguousarray(angles, np.float64).reshape(-1, 3)
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        s = None if sym is None else np.ascontiguousarray(sym, np.float64).reshape(-1, 9)
        self._insert(imgs, ctfs, ang, w, s, 0)
        self._calls.append((ang, w, s))

    def finish(self):
        L = lib()
        check(L.xh_rf2_weights_step(self.h, 0))
        for _ in range(1, self.niter):
            check(L.xh_rf2_weights_step(self.h, 1))
            for ang, w, s in self._calls:
                self._insert(None, None, ang, w, s, 1)
            check(L.xh_rf2_weights_step(self.h, 2))
        check(L.xh_rf2_weights_step(self.h, 3))
        out = np.empty((self.D,) * 3, np.float64)
        check(L.xh_rf2_finish(self.h, _np_ptr(out)))
        return out


def reduce_reconstructions(rfs):
    """Sum the cropped spaces of several handles of this process (one per device) into rfs[0]:
    the thread-per-device counterpart of allreduce_reconstruction (xh_rf_reduce)."""
    arr = (C.c_void_p * len(rfs))(*[r.h for r in rfs])
    check(lib().xh_rf_reduce(arr, len(rfs)))


def frc_dpr(ctx, m1, m2, sampling_rate=1.0, do_dpr=False, do_rfactor=False, min_freq=0.0, max_freq=0.5):
    """Fourier ring/shell correlation of two float64 device tensors of equal shape (2-D or 3-D): xh_frc_dpr,
    the core of xmipp_resolution_fsc (resolution_fsc.cpp:179-203). m1 is the reference map."""
    torch = _torch()
    assert m1.shape == m2.shape and m1.dtype == m2.dtype == torch.float64 and m1.is_cuda and m2.is_cuda
    m1, m2 = m1.contiguous(), m2.contiguous()
    shp = (1,) * (3 - m1.dim()) + tuple(m1.shape)
    L = shp[2] // 2 + 1
    out = {k: np.zeros(L) for k in ("freq", "frc", "frc_noise", "dpr", "error_l2")}
    rfac = np.full(1, -1.0)
    check(lib().xh_frc_dpr(ctx.h, _ptr(m1), _ptr(m2), shp[0], shp[1], shp[2], sampling_rate, int(do_dpr), int(do_rfactor),
                           min_freq, max_freq, _np_ptr(out["freq"]), _np_ptr(out["frc"]), _np_ptr(out["frc_noise"]),
                           _np_ptr(out["dpr"]), _np_ptr(out["error_l2"]), _np_ptr(rfac)))
    out["rfactor"] = float(rfac[0])
    return out


def allreduce_reconstruction(rf):
    """The one exchange step of the sharded path: SUM of [volume | weights] over ranks
    (replaces the per-row MPI_Reduce of parallel/mpi_reconstruct_fourier_accel.cpp:249-267)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(rf.cropped_view(), op=dist.ReduceOp.SUM)


class Fft2D(_Handle):
    """In-place complex 2-D FFT of an [ny, nx] complex64 cuda tensor, lines of any factorisable length (xh_fft2d_*: the
    four-step transform FlexAlign's movie frames need)."""

    _destroy = "xh_fft2d_destroy"

    def __init__(self, ctx, ny, nx):
        self.ctx, self.ny, self.nx = ctx, int(ny), int(nx)
        h = C.c_void_p()
        check(lib().xh_fft2d_create(ctx.h, self.ny, self.nx, C.byref(h)))
        super().__init__(ctx, h)
        f = np.zeros(4, np.int32)
        check(lib().xh_fft2d_factors(h, _np_ptr(f)))
        self.factors = tuple(int(v) for v in f)

    def __call__(self, data, inverse=False, axis=None):
        """Both axes (the inverse divided by ny nx), or one: axis 0 transforms the ny rows, axis 1 the nx columns (un-normalised
        in both directions)."""
        torch = _torch()
        assert data.is_cuda and data.dtype == torch.complex64 and data.is_contiguous() and tuple(data.shape) == (self.ny, self.nx)
        if axis is None:
            check(lib().xh_fft2d_exec(self.h, C.c_void_p(data.data_ptr()), int(bool(inverse))))
        else:
            check(lib().xh_fft2d_exec_axis(self.h, C.c_void_p(data.data_ptr()), int(bool(inverse)), int(axis)))
        return data

    # ---- test hook
    def debug_real_rows(self, frame, dark=None, gain=None, form=0, nc=0, out=None):
        """FlexAlign's row pass of a real [Y, X] frame on this plan (ny = (Y + 1) / 2, nx = X): form 0 -> ([ny, nx] complex64 in
        the four-step order, (n1, n2, done)), form 1 -> ([Y, nc] complex64, (n1, n2, done)). `out`: a complex64 cuda tensor of at
        least that many elements to write into."""
        torch = _torch()
        Y = frame.shape[0]
        assert all(a is None or tuple(a.shape) == (Y, self.nx) for a in (frame, dark, gain))
        shape = (self.ny, self.nx) if form == 0 else (Y, int(nc))
        if out is None:
            out = torch.zeros(shape, dtype=torch.complex64, device=frame.device)
        assert out.is_cuda and out.dtype == torch.complex64 and out.is_contiguous() and out.numel() >= shape[0] * shape[1]
        info = np.zeros(3, np.int32)
        check(lib().xh_fft2d_debug_real_rows(self.h, _ptr(frame, torch.float32), _ptr(dark, torch.float32), _ptr(gain, torch.float32), int(Y),
                                             int(nc), int(form), C.c_void_p(out.data_ptr()), _np_ptr(info)))
        return out, tuple(int(v) for v in info)


def debug_fft_lines(ctx, data, n, nlines, inner, outer_stride, inner_stride, elem_stride, max_lines=16, inverse=False):
    """Test hook: xh_plan.h's line transform in place on a complex64 (fp32) or complex128 (fp64) cuda tensor, strides in complex
    elements (xh_debug_fft_lines)."""
    torch = _torch()
    assert data.is_cuda and data.is_contiguous() and data.dtype in (torch.complex64, torch.complex128)
    if nlines > 0:        # the last element any line reaches lies inside the tensor
        last = (nlines - 1) // inner * outer_stride + (min(nlines, inner) - 1) * inner_stride + (n - 1) * elem_stride
        assert last < data.numel(), "the lines reach beyond the tensor"
    prec = 32 if data.dtype == torch.complex64 else 64
    check(lib().xh_debug_fft_lines(ctx.h, prec, int(n), C.c_void_p(data.data_ptr()), int(nlines), int(inner), int(outer_stride),
                                   int(inner_stride), int(elem_stride), int(max_lines), int(bool(inverse))))
    return data


class FlexAlign(_Handle):
    """Global alignment of a movie (ProgMovieAlignmentCorrelation*::computeGlobalAlignment) for frames of one size."""

    _destroy = "xh_fa_destroy"

    def __init__(self, ctx, Y, X, sampling_rate=1.0, max_res=30.0):
        self.ctx, self.Y, self.X = ctx, int(Y), int(X)
        h = C.c_void_p()
        check(lib().xh_fa_create(ctx.h, self.Y, self.X, float(sampling_rate), float(max_res), C.byref(h)))
        super().__init__(ctx, h)
        a, b, f = C.c_int32(), C.c_int32(), C.c_double()
        check(lib().xh_fa_info(h, C.byref(a), C.byref(b), C.byref(f)))
        self.new_dims, self.size_factor = (a.value, b.value), f.value

    def set_option(self, name, value):
        check(lib().xh_fa_set_option(self.h, name.encode(), float(value)))

    def last_full_pairs(self):
        return lib().xh_fa_last_full_pairs(self.h)

    def global_alignment(self, frames, max_shift_px, dark=None, gain=None):
        """frames [N, Y, X] float32 on the device -> dict(bX, bY, shiftX, shiftY, ref)"""
        torch = _torch()
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and tuple(frames.shape[1:]) == (self.Y, self.X)
        N = frames.shape[0]
        rows = N * (N - 1) // 2
        bx, by, sx, sy = np.empty(rows), np.empty(rows), np.empty(N), np.empty(N)
        ref = C.c_int32(0)
        check(lib().xh_fa_global_alignment(self.h, _ptr(frames), N, _ptr(dark, torch.float32), _ptr(gain, torch.float32), float(max_shift_px),
                                           _np_ptr(bx), _np_ptr(by), _np_ptr(sx), _np_ptr(sy), C.byref(ref)))
        return {"bX": bx, "bY": by, "shiftX": sx, "shiftY": sy, "ref": ref.value}

    def local_alignment(self, frames, g_shift_x, g_shift_y, ref, max_shift_px, patches=(7, 7), patch_size=(500, 500), patches_avg=3,
                        control_points=(6, 6, 5), dark=None, gain=None):
        """computeLocalAlignment of the CUDA program: dict(patch_shifts [py, px, N, 2], centers [py, px, 2], coeffsX, coeffsY, dims)"""
        torch = _torch()
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and tuple(frames.shape[1:]) == (self.Y, self.X)
        N = frames.shape[0]
        px, py = patches
        lX, lY, lT = control_points
        gx, gy = np.ascontiguousarray(g_shift_x, np.float64), np.ascontiguousarray(g_shift_y, np.float64)
        assert gx.shape == (N,) and gy.shape == (N,)
        shifts, centers = np.empty((py, px, N, 2)), np.empty((py, px, 2))
        cx, cy = np.empty(lX * lY * lT), np.empty(lX * lY * lT)
        dims = np.zeros(4, np.int32)
        check(lib().xh_fa_local_alignment(self.h, _ptr(frames), N, _ptr(dark, torch.float32), _ptr(gain, torch.float32), _np_ptr(gx), _np_ptr(gy), int(ref),
                                          float(max_shift_px), px, py, int(patch_size[0]), int(patch_size[1]), int(patches_avg), lX, lY, lT,
                                          _np_ptr(shifts), _np_ptr(centers), _np_ptr(cx), _np_ptr(cy), _np_ptr(dims)))
        return {"patch_shifts": shifts, "centers": centers, "coeffsX": cx, "coeffsY": cy, "dims": tuple(int(v) for v in dims)}

    def local_from_global(self, g_shift_x, g_shift_y, patches=(7, 7), patch_size=(500, 500), control_points=(6, 6, 5)):
        """localFromGlobal: the B-spline of a movie aligned globally only -> (coeffsX, coeffsY)"""
        gx, gy = np.ascontiguousarray(g_shift_x, np.float64), np.ascontiguousarray(g_shift_y, np.float64)
        N = gx.shape[0]
        px, py = patches
        lX, lY, lT = control_points
        centers = np.empty((py, px, 2))
        cx, cy = np.empty(lX * lY * lT), np.empty(lX * lY * lT)
        check(lib().xh_fa_local_from_global(self.h, N, _np_ptr(gx), _np_ptr(gy), px, py, int(patch_size[0]), int(patch_size[1]), lX, lY, lT, _np_ptr(centers),
                                            _np_ptr(cx), _np_ptr(cy)))
        return cx, cy

    def apply_bspline_frames(self, frames, coeffsX, coeffsY, control_points, n0=0, n1=None, dark=None, gain=None, out=None, total=None, initial=None):
        """Frames n0 .. n1 of frames [N, Y, X] warped by the B-spline in one call (the loop of applyShiftsComputeAverage): total += the
        aligned frames, initial += the corrected unaligned ones, out [n1 - n0 + 1, Y, X] = the aligned frames (each optional)."""
        torch = _torch()
        assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and tuple(frames.shape[1:]) == (self.Y, self.X)
        N = frames.shape[0]
        n1 = N - 1 if n1 is None else n1
        for t in (total, initial):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (self.Y, self.X))
        assert out is None or (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (n1 - n0 + 1, self.Y, self.X))
        lX, lY, lT = control_points
        cx, cy = np.ascontiguousarray(coeffsX, np.float64), np.ascontiguousarray(coeffsY, np.float64)
        assert cx.size == lX * lY * lT and cy.size == lX * lY * lT
        check(lib().xh_fa_apply_bspline_frames(self.h, _ptr(frames), N, int(n0), int(n1), _ptr(dark, torch.float32), _ptr(gain, torch.float32), _np_ptr(cx), _np_ptr(cy),
                                               lX, lY, lT, _ptr(out, torch.float32), _ptr(total, torch.float32), _ptr(initial, torch.float32)))

    def apply_bspline(self, frame, coeffsX, coeffsY, control_points, N, n, dark=None, gain=None, out=None, total=None, initial=None):
        """Frame n of N ([Y, X] float32 on the device) warped by the B-spline (applyBSplineTransform): out = aligned frame,
        total += it, initial += the corrected unaligned frame (each optional)."""
        torch = _torch()
        assert frame.is_cuda and frame.dtype == torch.float32 and frame.is_contiguous() and tuple(frame.shape) == (self.Y, self.X)
        for t in (out, total, initial):
            assert t is None or (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (self.Y, self.X))
        lX, lY, lT = control_points
        cx, cy = np.ascontiguousarray(coeffsX, np.float64), np.ascontiguousarray(coeffsY, np.float64)
        assert cx.size == lX * lY * lT and cy.size == lX * lY * lT
        check(lib().xh_fa_apply_bspline(self.h, _ptr(frame), _ptr(dark, torch.float32), _ptr(gain, torch.float32), _np_ptr(cx), _np_ptr(cy), lX, lY, lT, int(N), int(n),
                                        _ptr(out), _ptr(total), _ptr(initial)))
        return out


EXTREMA_MAX, EXTREMA_LOWEST, EXTREMA_MAX_AROUND_CENTER, EXTREMA_LOWEST_AROUND_CENTER = 0, 1, 2, 3


def extrema_find(ctx, data, search_type, max_dist=0.0):
    """SingleExtremaFinder on signals [n, (z,) (y,) x] float32 on the device -> (positions float32 [n], values float32 [n])"""
    torch = _torch()
    assert data.is_cuda and data.dtype == torch.float32 and data.is_contiguous() and 2 <= data.dim() <= 4
    shp = (data.shape[0],) + (1,) * (4 - data.dim()) + tuple(data.shape[1:])
    pos, val = np.empty(shp[0], np.float32), np.empty(shp[0], np.float32)
    check(lib().xh_extrema_find(ctx.h, _ptr(data), shp[0], shp[1], shp[2], shp[3], int(search_type), float(max_dist), _np_ptr(pos), _np_ptr(val)))
    return pos, val


def rotation_estimate(ctx, ref, others, first_ring=None, last_ring=None):
    """PolarRotationEstimator (OneToN): ref [D, D], others [n, D, D] float32 on the device -> rotations [n] in degrees as the
    reference returns them. Default rings: RotationEstimationSetting::getDefaultFirstRing / getDefaultLastRing."""
    torch = _torch()
    D = ref.shape[-1]
    assert ref.is_cuda and ref.dtype == torch.float32 and ref.is_contiguous() and tuple(ref.shape) == (D, D)
    assert others.is_cuda and others.dtype == torch.float32 and others.is_contiguous() and tuple(others.shape[1:]) == (D, D)
    if first_ring is None:
        first_ring = max(2, D // 20)
    if last_ring is None:
        last_ring = (D - 3) // 2
    out = np.empty(others.shape[0], np.float32)
    check(lib().xh_rotation_estimate(ctx.h, _ptr(ref), _ptr(others), others.shape[0], D, int(first_ring), int(last_ring), _np_ptr(out)))
    return out


def apply_geometry2d(ctx, src, matrices):
    """BSplineGeoTransformer::interpolate: src [n, y, x] float32 on the device, matrices [n, 3, 3] (applyGeometry LINEAR, IS_INV, DONT_WRAP)"""
    torch = _torch()
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3
    m = np.ascontiguousarray(matrices, np.float32).reshape(src.shape[0], 9)
    out = torch.empty_like(src)
    check(lib().xh_apply_geometry2d(ctx.h, _ptr(src), src.shape[0], src.shape[1], src.shape[2], _np_ptr(m), _ptr(out)))
    return out


def correlation_merit(ctx, ref, others):
    """CorrelationComputer (OneToN, normalised): correlationIndex(ref, others[i]) -> float32 [n]"""
    torch = _torch()
    assert ref.is_cuda and others.is_cuda and ref.dtype == others.dtype == torch.float32 and ref.is_contiguous() and others.is_contiguous()
    out = np.empty(others.shape[0], np.float32)
    check(lib().xh_correlation_merit(ctx.h, _ptr(ref), _ptr(others), others.shape[0], others.shape[1], others.shape[2], _np_ptr(out)))
    return out


def iterative_alignment(ctx, ref, others, max_shift, iters=3, first_ring=None, last_ring=None):
    """IterativeAlignmentEstimator::compute: ref [D, D], others [n, D, D] -> (poses [n, 3, 3] float32, merit [n])"""
    torch = _torch()
    D = ref.shape[-1]
    assert ref.is_cuda and ref.dtype == torch.float32 and ref.is_contiguous() and tuple(ref.shape) == (D, D)
    assert others.is_cuda and others.dtype == torch.float32 and others.is_contiguous() and tuple(others.shape[1:]) == (D, D)
    if first_ring is None:
        first_ring = max(2, D // 20)
    if last_ring is None:
        last_ring = (D - 3) // 2
    n = others.shape[0]
    poses, merit = np.empty((n, 9), np.float32), np.empty(n, np.float32)
    check(lib().xh_iterative_alignment(ctx.h, _ptr(ref), _ptr(others), n, D, int(max_shift), int(first_ring), int(last_ring), int(iters), _np_ptr(poses), _np_ptr(merit)))
    return poses.reshape(n, 3, 3), merit


class ShiftCorrEstimator(_Handle):
    """Alignment::ShiftCorrEstimator<float>, AlignType::OneToN, for images of x by y pixels (even)."""

    _destroy = "xh_shiftcorr_destroy"

    def __init__(self, ctx, x, y, max_shift):
        self.ctx, self.x, self.y = ctx, int(x), int(y)
        h = C.c_void_p()
        check(lib().xh_shiftcorr_create(ctx.h, self.x, self.y, int(max_shift), C.byref(h)))
        super().__init__(ctx, h)

    def load_reference(self, ref):
        torch = _torch()
        assert ref.is_cuda and ref.dtype == torch.float32 and ref.is_contiguous() and tuple(ref.shape) == (self.y, self.x)
        check(lib().xh_shiftcorr_load_reference(self.h, _ptr(ref)))

    def compute_shifts(self, others):
        """others [n, y, x] -> shifts [n, 2] (x, y) as getShifts2D returns them (the image's shift is the negative)"""
        torch = _torch()
        assert others.is_cuda and others.dtype == torch.float32 and others.is_contiguous() and tuple(others.shape[1:]) == (self.y, self.x)
        out = np.empty((others.shape[0], 2), np.float32)
        check(lib().xh_shiftcorr_compute_shifts(self.h, _ptr(others), others.shape[0], _np_ptr(out)))
        return out

    @staticmethod
    def correlate(ctx, inout, ref, center):
        """computeCorrelations2DOneToN: inout [n, fy, fx] complex64 <- ref conj(inout) (times (-1)^(x+y) when center), in place"""
        torch = _torch()
        assert inout.is_cuda and inout.dtype == torch.complex64 and inout.is_contiguous() and ref.dtype == torch.complex64 and ref.is_contiguous()
        assert tuple(ref.shape) == tuple(inout.shape[1:])
        check(lib().xh_shiftcorr_correlate(ctx.h, C.c_void_p(inout.data_ptr()), C.c_void_p(ref.data_ptr()), inout.shape[0], inout.shape[1], inout.shape[2], int(bool(center))))
        return inout


class AlignSignificant(_Handle):
    """The device side of xmipp_align_significant: every (reference, image) pair aligned with the chain of iterative_alignment, in
    batches of pairs; the significance weights; the weighted reference update. Defaults are the CUDA program's: max_shift D / 4, the
    default rings, iters 3."""

    _destroy = "xh_align_sig_destroy"

    def __init__(self, ctx, D, max_refs, batch_pairs=1024, max_shift=None, first_ring=None, last_ring=None, iters=3):
        self.ctx, self.D = ctx, int(D)
        if max_shift is None:
            max_shift = self.D // 4
        if first_ring is None:
            first_ring = max(2, self.D // 20)
        if last_ring is None:
            last_ring = (self.D - 3) // 2
        h = C.c_void_p()
        check(lib().xh_align_sig_create(ctx.h, self.D, int(max_refs), int(batch_pairs), int(max_shift), int(first_ring), int(last_ring), int(iters), C.byref(h)))
        super().__init__(ctx, h)
        self.R = 0

    def _images(self, t):
        torch = _torch()
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and tuple(t.shape[1:]) == (self.D, self.D)
        return t

    def load_references(self, refs):
        """refs [R, D, D] float32 on the device"""
        refs = self._images(refs)
        check(lib().xh_align_sig_load_references(self.h, _ptr(refs), refs.shape[0]))
        self.R = refs.shape[0]

    def align(self, images):
        """images [N, D, D] -> (poses [R, N, 3, 3], merit [R, N]) float32 tensors on the device"""
        torch = _torch()
        images = self._images(images)
        N = images.shape[0]
        poses = torch.empty((self.R, N, 3, 3), dtype=torch.float32, device=images.device)
        merit = torch.empty((self.R, N), dtype=torch.float32, device=images.device)
        check(lib().xh_align_sig_align(self.h, _ptr(images), N, _ptr(poses), _ptr(merit)))
        return poses, merit

    def weights(self, rot, tilt, ang_distance, merit):
        """computeWeightsAndSave: reference angles rot, tilt [R] (degrees), merit [R, N] on the device -> weights [R, N] on the device"""
        torch = _torch()
        assert merit.is_cuda and merit.dtype == torch.float32 and merit.is_contiguous() and merit.dim() == 2
        R, N = merit.shape
        rot, tilt = np.ascontiguousarray(rot, np.float32), np.ascontiguousarray(tilt, np.float32)
        assert rot.shape == (R,) and tilt.shape == (R,)
        out = torch.empty_like(merit)
        check(lib().xh_align_sig_weights(self.h, _np_ptr(rot), _np_ptr(tilt), float(ang_distance), _ptr(merit), R, N, _ptr(out)))
        return out

    def update_refs(self, images, ref_idx, img_idx, weight, pose, n_refs=None):
        """updateRefs: the assignments (ref_idx, img_idx, weight [n], pose [n, 3, 3]) -> the updated references [n_refs, D, D] on the
        device (n_refs: the number of references, by default the number loaded), each divided by the running sum of the weights of
        references 0 .. r (see include/xmipp_hip.h)"""
        R = self.R if n_refs is None else int(n_refs)
        torch = _torch()
        images = self._images(images)
        ref_idx, img_idx = np.ascontiguousarray(ref_idx, np.int32), np.ascontiguousarray(img_idx, np.int32)
        weight, pose = np.ascontiguousarray(weight, np.float32), np.ascontiguousarray(pose, np.float32).reshape(-1, 9)
        n = ref_idx.shape[0]
        assert img_idx.shape == (n,) and weight.shape == (n,) and pose.shape == (n, 9)
        out = torch.empty((R, self.D, self.D), dtype=torch.float32, device=images.device)
        check(lib().xh_align_sig_update_refs(self.h, _ptr(images), images.shape[0], R, n, _np_ptr(ref_idx), _np_ptr(img_idx), _np_ptr(weight), _np_ptr(pose), _ptr(out)))
        return out


class ReconstructSignificant(_Handle):
    """The device side of xmipp_reconstruct_significant: alignImagesConsideringMirrors of every (image, gallery projection) pair in
    double precision, in batches of chains (one chain = pair, mirror, order), the imed of every pair and the two significance
    weightings. See include/xmipp_hip.h for the arithmetic and the trace bits."""

    _destroy = "xh_rsig_destroy"
    STATS = ("steps", "shift_round1", "shift_round2", "shift_round3", "rotation_round1", "rotation_round2", "rotation_round3", "align_seconds",
             "image_weights_seconds", "direction_weights_seconds", "shift_steps_seconds", "rotation_steps_seconds",
             "neighbour_count_host_seconds")

    def __init__(self, ctx, D, max_gallery, batch_chains=4096):
        self.ctx, self.D = ctx, int(D)
        h = C.c_void_p()
        check(lib().xh_rsig_create(ctx.h, self.D, int(max_gallery), int(batch_chains), C.byref(h)))
        super().__init__(ctx, h)
        self.G = 0

    def _images(self, t):
        torch = _torch()
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 3 and tuple(t.shape[1:]) == (self.D, self.D)
        return t

    def load_gallery(self, gallery):
        """gallery [G, D, D] float64 on the device, G = volumes x directions"""
        gallery = self._images(gallery)
        check(lib().xh_rsig_load_gallery(self.h, _ptr(gallery), gallery.shape[0]))
        self.G = gallery.shape[0]

    def align(self, images, check_mirrors=True, trace=False, chains=False):
        """images [N, D, D] float64 -> (M [N, G, 3, 3], corr [N, G], imed [N, G]) float64 tensors on the device; with trace, the int32
        flags [N, G] as a fourth; with chains, a dict of every chain's M [N, G, mirrors, 2, 3, 3], corr, imed and trace as the last"""
        torch = _torch()
        images = self._images(images)
        N, G, dev = images.shape[0], self.G, images.device
        M = torch.empty((N, G, 3, 3), dtype=torch.float64, device=dev)
        corr = torch.empty((N, G), dtype=torch.float64, device=dev)
        imed = torch.empty((N, G), dtype=torch.float64, device=dev)
        tr = torch.empty((N, G), dtype=torch.int32, device=dev) if trace else None
        ch = None
        if chains:
            shape = (N, G, 2 if check_mirrors else 1, 2)
            ch = {"M": torch.empty(shape + (3, 3), dtype=torch.float64, device=dev), "corr": torch.empty(shape, dtype=torch.float64, device=dev),
                  "imed": torch.empty(shape, dtype=torch.float64, device=dev), "trace": torch.empty(shape, dtype=torch.int32, device=dev)}
        check(lib().xh_rsig_align(self.h, _ptr(images), N, int(bool(check_mirrors)), _ptr(M), _ptr(corr), _ptr(imed), _ptr(tr), _ptr(ch["M"]) if ch else None,
                                  _ptr(ch["corr"]) if ch else None, _ptr(ch["imed"]) if ch else None, _ptr(ch["trace"]) if ch else None))
        out = (M, corr, imed)
        if trace:
            out += (tr,)
        if chains:
            out += (ch,)
        return out

    def weights(self, M, cc, imed, n_vols, rot, tilt, ang_distance, one_alpha, apply_fisher=False, use_imed=False, strict=False, max_shift=-1.0):
        """Both weighting stages: M [N, G, 3, 3], cc and imed [N, G] float64 on the device (cc and imed take the maxShift penalty IN
        PLACE), direction angles rot, tilt [G] in degrees -> weight [N, G] on the device. one_alpha = 1 - alpha - deltaAlpha2.
        apply_fisher is the program's applyFisher, which its --dontApplyFisher switches ON (reconstruct_significant.cpp:88)."""
        torch = _torch()
        for t in (M, cc, imed):
            assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
        N, G = cc.shape
        assert tuple(M.shape) == (N, G, 3, 3) and tuple(imed.shape) == (N, G) and G % int(n_vols) == 0
        rot, tilt = np.ascontiguousarray(rot, np.float64), np.ascontiguousarray(tilt, np.float64)
        assert rot.shape == (G,) and tilt.shape == (G,)
        out = torch.empty_like(cc)
        check(lib().xh_rsig_weights(self.h, _ptr(M), _ptr(cc), _ptr(imed), N, int(n_vols), G // int(n_vols), _np_ptr(rot), _np_ptr(tilt), float(ang_distance),
                                    float(one_alpha), int(bool(apply_fisher)), int(bool(use_imed)), int(bool(strict)), float(max_shift), _ptr(out)))
        return out

    def set_timing(self, on):
        """a timed align waits for every step and reports the seconds inside shift and rotation steps"""
        check(lib().xh_rsig_set_timing(self.h, int(bool(on))))

    def stats(self):
        """of the last align and the last weights, a dict in the order of STATS"""
        v = np.zeros(len(self.STATS))
        check(lib().xh_rsig_stats(self.h, _np_ptr(v)))
        return dict(zip(self.STATS, v.tolist()))


class HalvesRestoration(_VolumeHandle):
    """The device side of xmipp_volume_halves_restoration (VolumeHalvesRestorator<double>): two half maps [Z, Y, X] float64 restored in
    place by denoise, deconvolve, filter_bank and difference, in that order, as the reference's apply runs them."""

    _destroy = "xh_halves_destroy"
    _PREFIX = "halves"

    OUTPUTS = ("restored1", "restored2", "filterBank", "deconvolved", "convolved", "avgDiff")

    def _mask(self, mask):
        return None if mask is None else _ptr(self._vol(mask, "mask", _torch().int32))

    def load(self, v1, v2):
        check(lib().xh_halves_load(self.h, _ptr(self._vol(v1)), _ptr(self._vol(v2))))

    def denoise(self, iters, mask=None):
        check(lib().xh_halves_denoise(self.h, int(iters), self._mask(mask)))

    def deconvolve(self, iters, sigma0=0.2, lam=0.001):
        """returns the (sigma1, sigma2) the Powell search chose in each iteration, [iters, 2]"""
        sig = np.zeros((max(1, int(iters)), 2))
        check(lib().xh_halves_deconvolve(self.h, int(iters), float(sigma0), float(lam), _np_ptr(sig)))
        return sig[:int(iters)]

    def filter_bank(self, step, overlap=0.5, weight_fun=1, weight_power=3.0):
        check(lib().xh_halves_filter_bank(self.h, float(step), float(overlap), int(weight_fun), float(weight_power)))

    def difference(self, iters, K=1.5, mask=None):
        check(lib().xh_halves_difference(self.h, int(iters), float(K), self._mask(mask)))

    def output(self, name):
        """one of OUTPUTS as a new device tensor, or None where its stage did not run"""
        out = self._new()
        present = C.c_int32()
        check(lib().xh_halves_output(self.h, self.OUTPUTS.index(name), _ptr(out), C.byref(present)))
        return out if present.value else None

    def deconv_spectra(self):
        check(lib().xh_halves_deconv_spectra(self.h))

    def sigma_cost(self, sigma1, sigma2):
        c = C.c_double()
        check(lib().xh_halves_sigma_cost(self.h, float(sigma1), float(sigma2), C.byref(c)))
        return c.value

    def rfft(self, v):
        """un-normalised r2c: [Z, Y, X] float64 -> [Z, Y, X // 2 + 1] complex128"""
        torch = _torch()
        Z, Y, X = self.shape
        out = torch.empty((Z, Y, X // 2 + 1), dtype=torch.complex128, device="cuda")
        check(lib().xh_halves_fft_r2c(self.h, _ptr(self._vol(v)), _ptr(out)))
        return out

    def irfft(self, F, scale=1.0):
        """un-normalised c2r times scale: [Z, Y, X // 2 + 1] complex128 -> [Z, Y, X] float64 (F is not modified)"""
        torch = _torch()
        Z, Y, X = self.shape
        assert F.is_cuda and F.dtype == torch.complex128 and F.is_contiguous() and tuple(F.shape) == (Z, Y, X // 2 + 1)
        out = self._new()
        check(lib().xh_halves_fft_c2r(self.h, _ptr(F), _ptr(out), float(scale)))
        return out

    def cdf(self, a, b=None, mask=None, mult=1.0):
        """Gpu::CDF table [202]: minimum, the 200 order statistics, maximum of a^2 or mult (a - b)^2 over the mask"""
        t = np.zeros(202)
        check(lib().xh_halves_cdf(self.h, _ptr(self._vol(a)), None if b is None else _ptr(self._vol(b)), self._mask(mask), float(mult), _np_ptr(t)))
        return t

    def set_timing(self, on):
        check(lib().xh_halves_set_timing(self.h, int(bool(on))))

    def band_timing(self):
        """(bands, [transforms, cdf, weights] ms summed over the last filter bank's bands)"""
        n = C.c_int32()
        ms = np.zeros(3)
        check(lib().xh_halves_band_timing(self.h, C.byref(n), _np_ptr(ms)))
        return n.value, ms


def halves_circular_mask(shape, R1, center=(0.0, 0.0, 0.0)):
    """the program's --mask circular R1 [--center x0 y0 z0] as an int32 array (host only)"""
    Z, Y, X = (int(s) for s in shape)
    m = np.zeros((Z, Y, X), np.int32)
    check(lib().xh_halves_circular_mask(Z, Y, X, float(R1), float(center[0]), float(center[1]), float(center[2]), _np_ptr(m)))
    return m


def halves_binary_mask(values):
    """the program's --mask binary_file: a file's float values -> int32 0 / 1 (host only)"""
    v = np.ascontiguousarray(values, np.float32)
    m = np.zeros(v.shape, np.int32)
    check(lib().xh_halves_binary_mask(_np_ptr(v), v.size, _np_ptr(m)))
    return m

class MonoRes(_StageTimes, _VolumeHandle):
    """The device side of xmipp_resolution_monogenic_signal (MonoRes): the local resolution map of a volume, or of two half maps,
    [Z, Y, X] float64 tensors on the device; masks are int32 tensors."""

    _destroy = "xh_mono_destroy"
    _PREFIX = "mono"

    STOP = {1: "range", 2: "mask_done", 3: "no_points", 4: "low_signal", 5: "ztest", 6: "min_res"}
    STAGES = ("split", "inverse", "rows", "smooth", "stats", "select", "assign")

    def run(self, vol, mask, vol2=None, mask_excl=None, sampling=1.0, min_res=30.0, max_res=1.0, step=0.25, significance=0.95, gaussian=False,
            noise_only_in_halves=False, max_steps=4096):
        """ProgMonogenicSignalRes::run. Returns a dict: mean (half maps only), refined_mask (int32), chimera, resolution_map (device
        tensors), steps (one dict per evaluated frequency), stop (why the sweep ended), radius, radiuslimit, nvoxels."""
        torch = _torch()
        from ._lib import MonoParams, MonoStep
        prm = MonoParams()
        lib().xh_mono_defaults(C.byref(prm))
        prm.sampling, prm.minRes, prm.maxRes, prm.freq_step, prm.significance = float(sampling), float(min_res), float(max_res), float(step), float(significance)
        prm.gaussian, prm.noise_only_in_halves = int(bool(gaussian)), int(bool(noise_only_in_halves))
        steps = (MonoStep * int(max_steps))()
        n, stop = C.c_int32(), C.c_int32()
        mean = self._new() if vol2 is not None else None
        refined = torch.empty(self.shape, dtype=torch.int32, device="cuda")
        chimera, resmap = self._new(), self._new()
        check(lib().xh_mono_run(self.h, _ptr(self._vol(vol)), None if vol2 is None else _ptr(self._vol(vol2, "second half")), _ptr(self._vol(mask, "mask", torch.int32)),
                                None if mask_excl is None else _ptr(self._vol(mask_excl, "exclusion mask", torch.int32)), C.byref(prm), C.cast(steps, C.c_void_p), int(max_steps),
                                C.byref(n), C.byref(stop), _ptr(mean), _ptr(refined), _ptr(chimera), _ptr(resmap)))
        recs = []
        for k in range(min(n.value, int(max_steps))):
            r = steps[k]
            rec = {f: getattr(r.stats, f) for f, _ in r.stats._fields_}
            rec.update({f: getattr(r, f) for f in ("resolution", "freq", "freqH", "freqL", "threshold", "z", "max_meanS", "assigned")})
            recs.append(rec)
        out = {"mean": mean, "refined_mask": refined, "chimera": chimera, "resolution_map": resmap, "steps": recs, "stop": self.STOP.get(stop.value, stop.value)}
        out.update(self.info())
        return out

    def info(self):
        r, rl, ns = C.c_int32(), C.c_int32(), C.c_int32()
        nv = C.c_int64()
        check(lib().xh_mono_info(self.h, C.byref(r), C.byref(rl), C.byref(nv), C.byref(ns)))
        return {"radius": r.value, "radiuslimit": rl.value, "nvoxels": nv.value, "nshell": ns.value}

    def amplitude(self, vol, freq, freqH, freqL, banded=True):
        """amplitudeMonoSig3D_LPF (banded) or monogenicAmplitude_3D_Fourier of a map, as a new device tensor"""
        out = self._new()
        check(lib().xh_mono_amplitude(self.h, _ptr(self._vol(vol)), float(freq), float(freqH), float(freqL), int(bool(banded)), _ptr(out)))
        return out

    def gaussian(self, vol, sigma):
        """realGaussianFilter of a copy of vol"""
        out = self._vol(vol).clone()
        check(lib().xh_mono_gaussian(self.h, _ptr(out), float(sigma)))
        return out

    def statistics(self, ampS, mask, ampN=None, significance=0.95):
        from ._lib import MonoStats
        st = MonoStats()
        check(lib().xh_mono_statistics(self.h, _ptr(self._vol(ampS, "amplitude")), None if ampN is None else _ptr(self._vol(ampN, "noise amplitude")), _ptr(self._vol(mask, "mask", _torch().int32)),
                                       float(significance), C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def select(self, vals, rank, mask=None):
        """element `rank` of the sorted values (of those whose mask is not 0); vals a 1-D float64 device tensor"""
        torch = _torch()
        assert vals.is_cuda and vals.dtype == torch.float64 and vals.is_contiguous() and vals.dim() == 1
        assert mask is None or (mask.is_cuda and mask.dtype == torch.int32 and mask.is_contiguous() and mask.shape == vals.shape)
        v = C.c_double()
        check(lib().xh_mono_select(self.h, _ptr(vals), _ptr(mask), vals.numel(), int(rank), C.byref(v)))
        return v.value

    def assign(self, amp, mask, res, threshold, resolution, resolution_2, halves):
        """the assign step on 1-D caller tensors, in place"""
        torch = _torch()
        assert amp.dtype == torch.float64 and res.dtype == torch.float64 and mask.dtype == torch.int32 and amp.numel() == mask.numel() == res.numel()
        check(lib().xh_mono_assign(self.h, _ptr(amp), _ptr(mask), _ptr(res), amp.numel(), float(threshold), float(resolution), float(resolution_2), int(bool(halves))))

    def shell_sums(self, vol):
        """findCliffValue's per-shell (sum, sum2, N) of a map about the Xmipp origin"""
        ns = self.info()["nshell"]
        s, s2, n = np.zeros(ns), np.zeros(ns), np.zeros(ns)
        check(lib().xh_mono_shell_sums(self.h, _ptr(self._vol(vol)), _np_ptr(s), _np_ptr(s2), _np_ptr(n)))
        return s, s2, n


def mono_icdf_gauss(p):
    """icdf_gauss as MonoRes uses it (host only)"""
    v = C.c_double()
    check(lib().xh_mono_icdf_gauss(float(p), C.byref(v)))
    return v.value


def mono_resolution_sweep(volsize, sampling, max_res, step, limit=100000):
    """resolution2eval called as run does until it breaks: the list of (decision, resolution, freq) with decision 'eval', 'continue' or
    'break' (host only; the sweep's other stop rules are not applied)"""
    count, last_idx, cont, brk = C.c_int32(0), C.c_int32(-1), C.c_int32(), C.c_int32()
    res, last, freq, freqL = C.c_double(), C.c_double(max_res), C.c_double(), C.c_double()
    out = []
    for _ in range(limit):
        check(lib().xh_mono_resolution2eval(C.byref(count), float(step), C.byref(res), C.byref(last), C.byref(freq), C.byref(freqL), C.byref(last_idx),
                                            int(volsize), C.byref(cont), C.byref(brk), float(sampling), float(max_res)))
        if cont.value:
            out.append(("continue", res.value, freq.value))
            continue
        if brk.value:
            out.append(("break", res.value, freq.value))
            break
        out.append(("eval", res.value, freq.value))
        last.value = res.value
    return out


def mono_cliff_radius(s, s2, n, radius, X):
    """the shell walk of findCliffValue over per-shell sums (host only)"""
    s, s2, n = (np.ascontiguousarray(a, np.float64) for a in (s, s2, n))
    out = C.c_int32()
    check(lib().xh_mono_cliff_radius(_np_ptr(s), _np_ptr(s2), _np_ptr(n), s.size, int(radius), int(X), C.byref(out)))
    return out.value


def mono_num_shells(shape):
    out = C.c_int32()
    check(lib().xh_mono_num_shells(*(int(v) for v in shape), C.byref(out)))
    return out.value


class LocalDeblur(_StageTimes, _VolumeHandle):
    """The device side of xmipp_volume_local_sharpening (LocalDeblur): sharpens a volume with its local resolution map, [Z, Y, X] float64
    tensors on the device. batch: the band spectra held at once (rounded up to an even number; any value gives the same bytes)."""

    _destroy = "xh_ldb_destroy"
    _PREFIX = "ldb"

    STAGES = ("forward", "split", "yz", "rows", "finish")

    def __init__(self, ctx, shape, batch=8):
        super().__init__(ctx, shape, int(batch))

    def load(self, vol, resmap, sampling=1.0, K=0.025):
        """produceSideInfo: the volume and its resolution map (both are copied)"""
        check(lib().xh_ldb_load(self.h, _ptr(self._vol(vol)), _ptr(self._vol(resmap, "resolution map")), float(sampling), float(K)))

    def info(self):
        """maxRes (before run's + 2), desvOutside, the number of voxels below 2 sampling and the band list: one dict per band with res, w,
        wL, idx and the kept lines of the y and z passes (kcount planes, jcount columns)"""
        mr, dv, no, nb = C.c_double(), C.c_double(), C.c_int64(), C.c_int32()
        check(lib().xh_ldb_info(self.h, C.byref(mr), C.byref(dv), C.byref(no), C.byref(nb), None, 0))
        b = np.zeros((nb.value, 6))
        check(lib().xh_ldb_info(self.h, None, None, None, None, _np_ptr(b), nb.value))
        bands = [{"res": r[0], "w": r[1], "wL": r[2], "idx": int(r[3]), "kcount": int(r[4]), "jcount": int(r[5])} for r in b]
        return {"maxRes": mr.value, "desvOutside": dv.value, "noutside": no.value, "bands": bands}

    def resmap(self):
        """the resolution map as load left it (clamped)"""
        out = self._new()
        check(lib().xh_ldb_resmap(self.h, _ptr(out)))
        return out

    def localfilter(self, v):
        """localfiltering of a volume, as a new device tensor"""
        out = self._new()
        check(lib().xh_ldb_localfilter(self.h, _ptr(self._vol(v)), _ptr(out)))
        return out

    def run(self, lam=1.0, niter=50):
        """ProgLocSharpening::run on the loaded volume: (sharpened map, lambda, one dict per iteration: norm, porc, subst, lambda, stop)"""
        from ._lib import LdbIter
        cap = max(int(niter), 1)
        recs = (LdbIter * cap)()
        n, stopped, lout = C.c_int32(), C.c_int32(), C.c_double()
        out = self._new()
        check(lib().xh_ldb_run(self.h, float(lam), int(niter), C.cast(recs, C.c_void_p), cap, C.byref(n), C.byref(stopped), C.byref(lout), _ptr(out)))
        its = [{"norm": r.norm, "porc": r.porc, "subst": r.subst, "lambda": r.lambda_, "stop": bool(r.stop)} for r in recs[:n.value]]
        return out, lout.value, its


def ldb_bands(zsize, sampling, max_res):
    """the bands of LocalDeblur's localfiltering for a spectrum of zsize planes, max_res being the loop's bound (the map's maximum + 2):
    a list of (res, w, wL, idx) (host only)"""
    n = C.c_int32()
    check(lib().xh_ldb_bands(int(zsize), float(sampling), float(max_res), None, 0, C.byref(n)))
    b = np.zeros((n.value, 4))
    check(lib().xh_ldb_bands(int(zsize), float(sampling), float(max_res), _np_ptr(b), n.value, C.byref(n)))
    return [(r[0], r[1], r[2], int(r[3])) for r in b]


class FSO(_StageTimes, _VolumeHandle):
    """The device side of xmipp_resolution_fso: global FSC, directional FSCs through Gaussian-weighted cones, FSO curve, 3DFSC of two
    half maps, [Z, Y, X] float64 tensors on the device. seg: the sorted coefficients a workgroup of the cone stage takes (0: the
    default); any value gives sums that differ in the last bits only, and the same bytes on every run."""

    _destroy = "xh_fso_destroy"
    _PREFIX = "fso"
    _WHAT = "half map"

    STAGES = ("transforms", "layout", "cones", "segment_reduce", "threedfsc")

    def __init__(self, ctx, shape, seg=0):
        super().__init__(ctx, shape, int(seg))
        self.L = self.shape[2] // 2 + 1

    def load(self, half1, half2, mask=None):
        """the transforms and the shell-sorted layout. Returns (sums [L, 3]: num, den1, den2 of the global FSC in fp64, the shells'
        sizes [L])"""
        sums, cnt, n = np.zeros((self.L, 3)), np.zeros(self.L, np.int64), C.c_int64()
        check(lib().xh_fso_load(self.h, _ptr(self._vol(half1)), _ptr(self._vol(half2)), None if mask is None else _ptr(self._vol(mask, "mask")), _np_ptr(sums),
                                _np_ptr(cnt), C.byref(n)))
        return sums, cnt

    def info(self):
        n, L, ns, seg = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().xh_fso_info(self.h, C.byref(n), C.byref(L), C.byref(ns), C.byref(seg)))
        return {"ncomps": n.value, "nshell": L.value, "nseg": ns.value, "seg": seg.value}

    def layout(self):
        """test hook: the sorted arrays as a dict of numpy arrays: fx, fy, fz, freqidx, arr2indx, real_z1z2, absz1, absz2"""
        n = self.info()["ncomps"]
        names = ("fx", "fy", "fz", "freqidx", "arr2indx", "real_z1z2", "absz1", "absz2")
        out = {k: np.zeros(n, np.int32 if k in ("freqidx", "arr2indx") else np.float32) for k in names}
        check(lib().xh_fso_layout(self.h, *(_np_ptr(out[k]) for k in names)))
        return out

    def directional(self, dirs, cos_angle, aux):
        """the cone sums of the unit vectors dirs [ndir, 3] (float32): (sums [ndir, L, 3] fp64, the coefficients inside each cone [ndir])"""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        sums, cnt = np.zeros((len(dirs), self.L, 3)), np.zeros(len(dirs), np.int64)
        check(lib().xh_fso_directional(self.h, _np_ptr(dirs), len(dirs), float(cos_angle), float(aux), _np_ptr(sums), _np_ptr(cnt)))
        return sums, cnt

    def threedfsc(self, dirs, cos_angle, aux, fsc, full=True):
        """the 3DFSC from the directional FSCs fsc [ndir, L] (float32): (half [Z, Y, X/2+1], full [Z, Y, X] or None), device tensors"""
        torch = _torch()
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        fsc = np.ascontiguousarray(fsc, np.float32)
        if fsc.shape != (len(dirs), self.L):
            raise XhError(f"FSO: the directional FSCs have shape {fsc.shape}, expected {(len(dirs), self.L)}")
        Z, Y, X = self.shape
        half = torch.empty((Z, Y, X // 2 + 1), dtype=torch.float64, device="cuda")
        out = self._new() if full else None
        check(lib().xh_fso_threedfsc(self.h, _np_ptr(dirs), len(dirs), float(cos_angle), float(aux), _np_ptr(fsc), _ptr(half), _ptr(out)))
        return half, out

    def run(self, half1, half2, mask=None, sampling=1.0, anglecone=17.0, threshold=0.143, threedfsc=False, level=3, distribution=True):
        """ProgFSO::run. Returns a dict: global_sums, global_fsc (num / sqrt(den1 den2)), freq, directions (degrees), dirs, fsc (directional,
        float32), resolution (per direction), fso, bingham, anisotropy (the table's value), counts, distribution [360, 91] (or None),
        and with threedfsc the device tensors threedfsc_half and threedfsc_full"""
        sums, _ = self.load(half1, half2, mask)
        ang = fso_directions(level)
        dirs = fso_unit_vectors(ang)
        cos_angle, aux = fso_cone(anglecone)
        dsums, counts = self.directional(dirs, cos_angle, aux)
        fsc, resol, fso, bingham = fso_decide(dsums, dirs, self.shape[2], sampling, threshold)
        with np.errstate(divide="ignore", invalid="ignore"):
            gfsc = sums[:, 0] / np.sqrt(sums[:, 1] * sums[:, 2])
        out = {"global_sums": sums, "global_fsc": gfsc, "freq": np.arange(self.L, dtype=np.float32).astype(np.float64) / (self.shape[2] * float(sampling)),
               "directions": ang, "dirs": dirs, "fsc": fsc, "resolution": resol, "fso": fso, "bingham": bingham,
               "anisotropy": np.array([fso_incomplete_gamma(b) for b in bingham]), "counts": counts,
               "distribution": fso_resolution_distribution(dirs, resol, anglecone) if distribution else None}
        if threedfsc:
            out["threedfsc_half"], out["threedfsc_full"] = self.threedfsc(dirs, cos_angle, aux, fsc)
        return out


class VolumeSubtraction(_StageTimes, _VolumeHandle):
    """The device side of xmipp_volume_subtraction: a volume is adjusted to a reference by projections onto convex sets, and the
    reference minus the adjusted volume is formed inside a mask. [Z, Y, X] float64 tensors on the device; spectra are [Z, Y, X // 2 + 1]."""

    _destroy = "xh_vsub_destroy"
    _PREFIX = "vsub"

    STAGES = ("transforms", "spectrum", "real", "filter")
    ENERGIES = ("amplitude", "minmax", "mask", "phase", "nonneg", "scale", "filter")

    def __init__(self, ctx, shape):
        super().__init__(ctx, shape)
        self.half_shape = self.shape[:2] + (self.shape[2] // 2 + 1,)

    def set_reference(self, v1, mask=None, radavg=False):
        """the reference volume and the mask (None: ones; the product of both masks, as the reference uses a mask only when it has
        both). radavg: also V1's radial mean, which adjust(radavg=True) needs"""
        m = None if mask is None else _ptr(self._vol(mask, "mask"))
        check(lib().xh_vsub_set_reference(self.h, _ptr(self._vol(v1, "reference")), m, int(bool(radavg))))

    def info(self):
        """v1min, v1max, std1 of the masked, clipped reference and the number of radial bins"""
        lo, hi, sd, nb = C.c_double(), C.c_double(), C.c_double(), C.c_int32()
        check(lib().xh_vsub_info(self.h, C.byref(lo), C.byref(hi), C.byref(sd), C.byref(nb)))
        return {"v1min": lo.value, "v1max": hi.value, "std1": sd.value, "nbins": nb.value}

    def reference_magnitude(self):
        """V1FourierMag"""
        out = _torch().empty(self.half_shape, dtype=_torch().float64, device="cuda")
        check(lib().xh_vsub_reference_magnitude(self.h, _ptr(out)))
        return out

    def radial_mean(self, mag):
        """radialAverage of a magnitude [Z, Y, X // 2 + 1], as a numpy array [nbins]"""
        out = np.zeros(vsub_radial_bins(self.shape)[0])
        check(lib().xh_vsub_radial_mean(self.h, _ptr(self._vol(mag, "magnitude", shape=self.half_shape)), _np_ptr(out)))
        return out

    def quotient(self, v):
        """computeRadQuotient of the reference against the volume v as it is, as a numpy array [nbins]"""
        out = np.zeros(vsub_radial_bins(self.shape)[0])
        check(lib().xh_vsub_quotient(self.h, _ptr(self._vol(v)), _np_ptr(out)))
        return out

    def iteration(self, v0, v, lam=1.0, radavg=False, cut_freq=0.0):
        """one runIteration of v with the phases (and the quotient) of v0"""
        out = self._new()
        check(lib().xh_vsub_iteration(self.h, _ptr(self._vol(v0)), _ptr(self._vol(v)), float(lam), int(bool(radavg)), float(cut_freq), _ptr(out)))
        return out

    def adjust(self, v, niter=5, lam=1.0, radavg=False, cut_freq=0.0, energies=False):
        """the adjusted volume; with energies also one dict per iteration with the RMS change over each step"""
        from ._lib import VsubEnergy
        out = self._new()
        recs = (VsubEnergy * max(int(niter), 1))() if energies else None
        check(lib().xh_vsub_adjust(self.h, _ptr(self._vol(v)), int(niter), float(lam), int(bool(radavg)), float(cut_freq),
                                   C.cast(recs, C.c_void_p) if energies else None, _ptr(out)))
        if not energies:
            return out
        return out, [{k: getattr(r, k) for k in self.ENERGIES} for r in recs[:max(int(niter), 0)]]

    def lowpass(self, v, cut_freq):
        out = self._new()
        check(lib().xh_vsub_lowpass(self.h, _ptr(self._vol(v)), float(cut_freq), _ptr(out)))
        return out

    def smooth_mask(self, mask, sigma=3):
        """the mask through the REALGAUSSIAN low pass with w1 = sigma"""
        out = self._new()
        check(lib().xh_vsub_smooth_mask(self.h, _ptr(self._vol(mask, "mask")), float(sigma), _ptr(out)))
        return out

    def subtract(self, v1_raw, vadj, masksub, cut_freq=0.0):
        """(V1 (1 - m) + (V1F - min(Vadj, V1F)) m, V1F)"""
        out, v1f = self._new(), self._new()
        check(lib().xh_vsub_subtract(self.h, _ptr(self._vol(v1_raw, "reference")), _ptr(self._vol(vadj, "adjusted volume")),
                                     _ptr(self._vol(masksub, "subtraction mask")), float(cut_freq), _ptr(v1f), _ptr(out)))
        return out, v1f


class Symmetrize(_StageTimes, _VolumeHandle):
    """The device side of xmipp_transform_symmetrize: a volume through a point group or a helix, an image stack through a rotation order,
    and xmippCore's 3-D applyGeometry and spline coefficients under them. float64 tensors on the device; a shape (1, Y, X) makes a handle for
    image stacks [n, Y, X], any other a handle for volumes [Z, Y, X]."""

    _destroy = "xh_sym_destroy"
    _PREFIX = "sym"

    STAGES = ("coefficients", "outside_mean", "pass")

    def set_matrices(self, R):
        """the R of SymList::getMatrices, [n, 3, 3] on the host, identity excluded"""
        R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3))
        check(lib().xh_sym_set_matrices(self.h, _np_ptr(R), len(R)))
        self.n_matrices = len(R)

    def symmetrize(self, v, degree=3, wrap=True, sum=False):
        """symmetrizeVolume over the matrices set: (V + sum_i applyGeometry(V, R_i^T)) / (n + 1), or the sum alone"""
        out = self._new()
        check(lib().xh_sym_symmetrize(self.h, _ptr(self._vol(v)), int(degree), int(bool(wrap)), int(bool(sum)), _ptr(out)))
        return out

    def symmetrize_images(self, imgs, order, degree=3, wrap=True, sum=False):
        """symmetrizeImage of every image of a stack [n, Y, X] (a handle of shape (1, Y, X))"""
        n = int(imgs.shape[0])
        self._vol(imgs, "stack", shape=(n,) + self.shape[1:])
        out = _torch().empty_like(imgs)
        check(lib().xh_sym_symmetrize_images(self.h, _ptr(imgs), n, int(order), int(degree), int(bool(wrap)), int(bool(sum)), _ptr(out)))
        return out

    def helical(self, v, z_helical, rot_helical, rot_phase=0.0, cn=1, dihedral=False, height_fraction=0.95, degree=3):
        """symmetry_Helical; z_helical in voxels, the angles in radians. dihedral: the helicalDihedral branch of symmetrizeVolume"""
        out = self._new()
        check(lib().xh_sym_helical(self.h, _ptr(self._vol(v)), float(z_helical), float(rot_helical), float(rot_phase), int(cn), int(bool(dihedral)),
                                   float(height_fraction), int(degree), _ptr(out)))
        return out

    def apply_geometry3d(self, v, A, degree=3, wrap=True, outside=0.0):
        """applyGeometry(degree, ., V, A, IS_NOT_INV, wrap, outside) for one 3 x 3 matrix on the host"""
        A = np.ascontiguousarray(np.asarray(A, dtype=np.float64).reshape(3, 3))
        out = self._new()
        check(lib().xh_sym_apply_geometry3d(self.h, _ptr(self._vol(v)), _np_ptr(A), int(degree), int(bool(wrap)), float(outside), _ptr(out)))
        return out

    def coefficients(self, v):
        """produceSplineCoefficients(BSPLINE3) of a volume"""
        out = self._new()
        check(lib().xh_sym_coefficients(self.h, _ptr(self._vol(v)), _ptr(out)))
        return out

    def outside_mean(self, v):
        """the mean over r^2 >= (min(shape) // 2)^2"""
        m = C.c_double()
        check(lib().xh_sym_outside_mean(self.h, _ptr(self._vol(v)), C.byref(m)))
        return m.value


def sym_helical_depth(Z, z_helical, height_fraction=0.95, dihedral=False):
    """the depth the helical interpolation's recursion reaches on Z planes: 0 or 1, or -1 where Symmetrize.helical refuses (host only)"""
    depth = C.c_int32()
    check(lib().xh_sym_helical_depth(int(Z), float(z_helical), float(height_fraction), int(bool(dihedral)), C.byref(depth)))
    return depth.value


class VolumeAlign(_StageTimes, _VolumeHandle):
    """The device side of xmipp_volume_align: the fitness of many trials per pass over V1 and the mask. A trial is the reference's
    10-vector (flip, greyScale, greyShift, rot, tilt, psi, scale, z, y, x); volumes, masks and trials come from the host as numpy arrays.
    capacity: the most trials of one launch; no result depends on it."""

    _destroy = "xh_valign_destroy"
    _PREFIX = "valign"

    STAGES = ("gather", "finish", "select")
    COVARIANCE, LEAST_SQUARES = 1, 2

    def __init__(self, ctx, shape, capacity=256):
        super().__init__(ctx, shape, int(capacity))
        self.capacity = int(capacity)

    def set_volumes(self, V1, V2, mask=None):
        """V1 (fixed) and V2 (moved), float64 [Z, Y, X]; mask: int32, nonzero = inside, or None"""
        V1 = np.ascontiguousarray(V1, np.float64)
        V2 = np.ascontiguousarray(V2, np.float64)
        if V1.shape != self.shape or V2.shape != self.shape:
            raise XhError(f"VolumeAlign: volumes of shape {V1.shape} and {V2.shape}, the handle {self.shape}")
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.int32)
            if mask.shape != self.shape:
                raise XhError(f"VolumeAlign: the mask has shape {mask.shape}, the handle {self.shape}")
        check(lib().xh_valign_set_volumes(self.h, _np_ptr(V1), _np_ptr(V2), _np_ptr(mask)))

    def stats(self):
        """(n, mean_x, stddev_x, sum (x - mean_x)) of V1 within the mask"""
        s = np.zeros(4)
        check(lib().xh_valign_stats(self.h, _np_ptr(s)))
        return tuple(s)

    @staticmethod
    def _trials(p):
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 10))

    def fit(self, trials, method=1, wrap=True):
        """fitness of every trial [m, 10]: minus correlationIndex (method 1) or rms (method 2) of V1 against the transformed V2"""
        p = self._trials(trials)
        out = np.zeros(len(p))
        check(lib().xh_valign_fit(self.h, _np_ptr(p), len(p), int(method), int(bool(wrap)), _np_ptr(out)))
        return out

    def search(self, trials, method=1, wrap=True, fits=False):
        """(index, fit) of the first minimum in trial order; with fits=True also every trial's fit"""
        p = self._trials(trials)
        out = np.zeros(len(p)) if fits else None
        idx, best = C.c_int64(), C.c_double()
        check(lib().xh_valign_search(self.h, _np_ptr(p), len(p), int(method), int(bool(wrap)), C.byref(idx), C.byref(best), _np_ptr(out)))
        return (idx.value, best.value, out) if fits else (idx.value, best.value)

    def apply(self, trial, wrap=True):
        """applyTransformation(V2, trial, wrap) as a float64 device tensor"""
        p = self._trials(trial)
        assert len(p) == 1
        out = self._new()
        check(lib().xh_valign_apply(self.h, _np_ptr(p), int(bool(wrap)), _ptr(out)))
        return out

    @staticmethod
    def matrix(trial):
        """(A, Ainv, isIdentity) of a trial: 4 x 4 arrays (host only)"""
        p = np.ascontiguousarray(trial, np.float64).reshape(10)
        A, Ai, ident = np.zeros((4, 4)), np.zeros((4, 4)), C.c_int32()
        check(lib().xh_valign_matrix(_np_ptr(p), _np_ptr(A), _np_ptr(Ai), C.byref(ident)))
        return A, Ai, bool(ident.value)


def valign_trials(ranges, consider_mirror=False, limit=1 << 21):
    """the exhaustive search's trials [count, 10] in the reference's order and its progress-bar count (host only). ranges: (first, last,
    step) of grey_scale, grey_shift, rot, tilt, psi, scale, z, y, x"""
    r = np.ascontiguousarray(ranges, np.float64).reshape(9, 3)
    n, times = C.c_int64(), C.c_int64()
    check(lib().xh_valign_trials(_np_ptr(r), int(bool(consider_mirror)), int(limit), None, C.byref(n), C.byref(times)))
    p = np.zeros((n.value, 10))
    check(lib().xh_valign_trials(_np_ptr(r), int(bool(consider_mirror)), int(limit), _np_ptr(p), C.byref(n), None))
    return p, times.value


class FindSymmetry(_StageTimes, _VolumeHandle):
    """The device side of xmipp_volume_find_symmetry: the correlation of a volume with its own symmetrised copy for many trials per pass
    over the volume and the mask. Axis trials are (rot, tilt) in degrees; helical trials are (rot in degrees, z in voxels), the order of
    the reference's Powell vector. The volume, the mask and the trials come from the host as numpy arrays. capacity: the most trials of
    one launch; no result depends on it."""

    _destroy = "xh_fsym_destroy"
    _PREFIX = "fsym"

    STAGES = ("gather", "finish", "select")
    GATED = -1e38

    def __init__(self, ctx, shape, capacity=256):
        super().__init__(ctx, shape, int(capacity))
        self.capacity = int(capacity)

    def set_volume(self, V, mask=None, splines=False):
        """V float64 [Z, Y, X]; mask: int32, nonzero = inside, or None; splines: --useSplines for the axis fits"""
        V = np.ascontiguousarray(V, np.float64)
        if V.shape != self.shape:
            raise XhError(f"FindSymmetry: a volume of shape {V.shape}, the handle {self.shape}")
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.int32)
            if mask.shape != self.shape:
                raise XhError(f"FindSymmetry: the mask has shape {mask.shape}, the handle {self.shape}")
        check(lib().xh_fsym_set_volume(self.h, _np_ptr(V), _np_ptr(mask), int(bool(splines))))

    def stats(self, clipped=False):
        """(n, mean, stddev, sum (x - mean)) of V within the mask; clipped: within the mask of the last helical fit"""
        s = np.zeros(4)
        check(lib().xh_fsym_stats(self.h, int(bool(clipped)), _np_ptr(s)))
        return tuple(s)

    @staticmethod
    def _trials(p):
        return np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1, 2))

    @staticmethod
    def _box(box):
        return None if box is None else np.ascontiguousarray(box, np.float64).reshape(4)

    def axis_fit(self, trials, rot_sym):
        """correlationIndex(V, V + sum_n applyGeometry(V, A_n), mask) of every trial [m, 2]"""
        p = self._trials(trials)
        out = np.zeros(len(p))
        check(lib().xh_fsym_axis_fit(self.h, _np_ptr(p), len(p), int(rot_sym), _np_ptr(out)))
        return out

    def axis_search(self, trials, rot_sym, corrs=False):
        """(index, corr) of the first trial above every one before it and above 0; (-1, 0.0) where no correlation is above 0. With
        corrs=True also every trial's correlation"""
        p = self._trials(trials)
        out = np.zeros(len(p)) if corrs else None
        idx, best = C.c_int64(), C.c_double()
        check(lib().xh_fsym_axis_search(self.h, _np_ptr(p), len(p), int(rot_sym), C.byref(idx), C.byref(best), _np_ptr(out)))
        return (idx.value, best.value, out) if corrs else (idx.value, best.value)

    def helical_fit(self, trials, box=None, dihedral=False, height_fraction=1.0, cn=1):
        """the correlation of every trial [m, 2] = (rot, z); box = (z0, zF, rot0, rotF): trials the reference's gate refuses get GATED"""
        p, b = self._trials(trials), self._box(box)
        out = np.zeros(len(p))
        check(lib().xh_fsym_helical_fit(self.h, _np_ptr(p), len(p), _np_ptr(b), int(bool(dihedral)), float(height_fraction), int(cn), _np_ptr(out)))
        return out

    def helical_search(self, trials, box=None, dihedral=False, height_fraction=1.0, cn=1, corrs=False):
        p, b = self._trials(trials), self._box(box)
        out = np.zeros(len(p)) if corrs else None
        idx, best = C.c_int64(), C.c_double()
        check(lib().xh_fsym_helical_search(self.h, _np_ptr(p), len(p), _np_ptr(b), int(bool(dihedral)), float(height_fraction), int(cn), C.byref(idx),
                                           C.byref(best), _np_ptr(out)))
        return (idx.value, best.value, out) if corrs else (idx.value, best.value)

    def axis_volume(self, rot, tilt, rot_sym):
        """the materialised volume_sym of one axis trial as a float64 device tensor (a test hook)"""
        out = self._new()
        check(lib().xh_fsym_axis_volume(self.h, float(rot), float(tilt), int(rot_sym), _ptr(out)))
        return out

    def helical_volume(self, rot, z, dihedral=False, height_fraction=1.0, cn=1):
        """symmetry_Helical's masked output of one trial as a float64 device tensor (a test hook)"""
        out = self._new()
        check(lib().xh_fsym_helical_volume(self.h, float(rot), float(z), int(bool(dihedral)), float(height_fraction), int(cn), _ptr(out)))
        return out


def fsym_axis_matrices(rot, tilt, rot_sym):
    """(A, Ainv) [rot_sym - 1, 3, 3]: rotation3DMatrix(360 / rot_sym * n, row 2 of Euler(rot, tilt, 0)) and the inverses (host only)"""
    n = min(max(int(rot_sym) - 1, 1), 98)                   # an order outside 2 .. 99 is refused by the library
    A, Ai = np.zeros((n, 3, 3)), np.zeros((n, 3, 3))
    check(lib().xh_fsym_axis_matrices(float(rot), float(tilt), int(rot_sym), _np_ptr(A), _np_ptr(Ai)))
    return A, Ai


def fsym_grid(range0, range1, limit=1 << 21):
    """the two nested loops of an exhaustive search: (trials [count, 2], n_outer, n_inner); ranges are (first, last, step) (host only)"""
    a = [float(v) for v in range0] + [float(v) for v in range1]
    n, no, ni = C.c_int64(), C.c_int64(), C.c_int64()
    check(lib().xh_fsym_grid(*a, int(limit), None, C.byref(n), C.byref(no), C.byref(ni)))
    p = np.zeros((n.value, 2))
    check(lib().xh_fsym_grid(*a, int(limit), _np_ptr(p), C.byref(n), C.byref(no), C.byref(ni)))
    return p, no.value, ni.value


def fsym_helical_gate(Z, z_helical, rot_helical, z0, zF, rot0, rotF):
    """True where evaluateSymmetry returns 1e38 without any work (host only)"""
    g = C.c_int32()
    check(lib().xh_fsym_helical_gate(int(Z), float(z_helical), float(rot_helical), float(z0), float(zF), float(rot0), float(rotF), C.byref(g)))
    return bool(g.value)


def fsym_helical_depth(Z, z_helical, height_fraction=1.0, dihedral=False):
    """the depth the helical interpolation's recursion reaches for FindSymmetry's masked helix: 0 or 1, or -1 where it is refused (host only)"""
    depth = C.c_int32()
    check(lib().xh_fsym_helical_depth(int(Z), float(z_helical), float(height_fraction), int(bool(dihedral)), C.byref(depth)))
    return depth.value


def halves_cylinder_mask(shape, R, H, center=(0.0, 0.0, 0.0)):
    """--mask cylinder R H [--center x0 y0 z0] as an int32 array: both negative keep the inside (host only)"""
    Z, Y, X = (int(s) for s in shape)
    m = np.zeros((Z, Y, X), np.int32)
    check(lib().xh_halves_cylinder_mask(Z, Y, X, float(R), float(H), float(center[0]), float(center[1]), float(center[2]), _np_ptr(m)))
    return m


def halves_tube_mask(shape, R1, R2, H, center=(0.0, 0.0, 0.0)):
    """--mask tube R1 R2 H [--center x0 y0 z0] as an int32 array: all negative keep the inside (host only)"""
    Z, Y, X = (int(s) for s in shape)
    m = np.zeros((Z, Y, X), np.int32)
    check(lib().xh_halves_tube_mask(Z, Y, X, float(R1), float(R2), float(H), float(center[0]), float(center[1]), float(center[2]), _np_ptr(m)))
    return m


def vsub_radial_bins(shape):
    """(the bins of the radial average of a [Z, Y, X] box, the largest bin its octant writes); --radavg is refused where the second
    reaches the first (host only)"""
    nb, mb = C.c_int32(), C.c_int32()
    check(lib().xh_vsub_radial_bins(*(int(v) for v in shape), C.byref(nb), C.byref(mb)))
    return nb.value, mb.value


def fso_directions(level=3):
    """the direction set of xmipp_resolution_fso: (rot, tilt) in degrees, float32 [n, 2]; level 3 gives 321, level 2 81 (host only)"""
    n = C.c_int32()
    check(lib().xh_fso_directions(int(level), None, 0, C.byref(n)))
    a = np.zeros((n.value, 2), np.float32)
    check(lib().xh_fso_directions(int(level), _np_ptr(a), n.value, C.byref(n)))
    return a


def fso_unit_vectors(rot_tilt_deg):
    """the float unit vectors the cones use, from (rot, tilt) in degrees: float32 [n, 3] (host only)"""
    a = np.ascontiguousarray(rot_tilt_deg, np.float32).reshape(-1, 2)
    out = np.zeros((len(a), 3), np.float32)
    check(lib().xh_fso_unit_vectors(_np_ptr(a), len(a), _np_ptr(out)))
    return out


def fso_incomplete_gamma(x):
    """the reference's table of the incomplete gamma function P(5, x), indexed by round(2 x) clamped to 0 .. 40 (host only)"""
    return lib().xh_fso_incomplete_gamma(float(x))


def fso_cone(anglecone):
    """(cosAngle, aux) of a cone of `anglecone` degrees, as floats (host only)"""
    c, a = C.c_float(), C.c_float()
    check(lib().xh_fso_cone(float(anglecone), C.byref(c), C.byref(a)))
    return c.value, a.value


def fso_decide(dsums, dirs, xdim, sampling=1.0, threshold=0.143):
    """the host decisions on the cone sums [ndir, L, 3]: (fsc float32 [ndir, L], resolution [ndir], fso float32 [L], bingham [L]) (host only)"""
    dsums = np.ascontiguousarray(dsums, np.float64)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    ndir, L = dsums.shape[:2]
    assert dsums.shape == (len(dirs), L, 3)
    fsc, resol, fso, bingham = np.zeros((ndir, L), np.float32), np.zeros(ndir), np.zeros(L, np.float32), np.zeros(L)
    check(lib().xh_fso_decide(_np_ptr(dsums), _np_ptr(dirs), ndir, L, int(xdim), float(sampling), float(threshold), _np_ptr(fsc), _np_ptr(resol), _np_ptr(fso),
                              _np_ptr(bingham)))
    return fsc, resol, fso, bingham


def fso_resolution_distribution(dirs, resol, anglecone):
    """resolutionDistribution: the weighted directional resolution on the grid rot 0 .. 359, tilt 0 .. 90: [360, 91] (host only)"""
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    resol = np.ascontiguousarray(resol, np.float64)
    out = np.zeros((360, 91))
    check(lib().xh_fso_resolution_distribution(_np_ptr(dirs), len(dirs), _np_ptr(resol), float(anglecone), _np_ptr(out)))
    return out


def vds_num_terms(L1, L2):
    """terms of the Zernike3D basis of degrees (L1, L2) (host only)"""
    n = C.c_int32()
    check(lib().xh_vds_num_terms(int(L1), int(L2), C.byref(n)))
    return n.value


def vds_terms(L1, L2):
    """the basis terms (l1, n, l2, m) of degrees (L1, L2), int32 [n, 4] (host only)"""
    out = np.zeros((vds_num_terms(L1, L2), 4), np.int32)
    check(lib().xh_vds_terms(int(L1), int(L2), _np_ptr(out)))
    return out


def vds_zsh(l1, n, l2, m, xr, yr, zr, r):
    """one basis term at one point, by the function the kernels run (host only)"""
    v = C.c_double()
    check(lib().xh_vds_zsh(int(l1), int(n), int(l2), int(m), float(xr), float(yr), float(zr), float(r), C.byref(v)))
    return v.value


class ReconstructWbp(_StageTimes, _VolumeHandle):
    """The device side of xmipp_reconstruct_wbp: weighted back-projection with the arbitrary-geometry filter. The caller forms the
    direction list mat_g and every image's two matrices on the host; images are float32 [n, D, D] numpy arrays. capacity: the images of
    one batch; no result depends on it."""

    _destroy = "xh_wbp_destroy"
    _PREFIX = "wbp"

    STAGES = ("prepare", "transforms", "filter", "backprojection", "finish")
    ROW = 22

    def __init__(self, ctx, D, capacity=64):
        self.ctx = ctx
        self.D, self.capacity = int(D), int(capacity)
        self.shape = (self.D,) * 3
        h = C.c_void_p()
        check(lib().xh_wbp_create(ctx.h, self.D, self.capacity, C.byref(h)))
        _Handle.__init__(self, ctx, h)

    @staticmethod
    def rows(shifts_x, shifts_y, flips, weights, filter_matrices, backprojection_matrices):
        """[n, 22] rows of add(): shiftX, shiftY, flip, weight, Euler_angles2matrix(-rot, tilt, -psi), inv(Euler_angles2matrix(rot, -tilt, psi))"""
        n = len(shifts_x)
        r = np.zeros((n, 22))
        r[:, 0], r[:, 1], r[:, 2], r[:, 3] = shifts_x, shifts_y, np.asarray(flips, dtype=bool), weights
        r[:, 4:13] = np.asarray(filter_matrices, dtype=np.float64).reshape(n, 9)
        r[:, 13:22] = np.asarray(backprojection_matrices, dtype=np.float64).reshape(n, 9)
        return r

    def reset(self):
        """a new reconstruction: zero volume, zero count_thr; the directions stay"""
        check(lib().xh_wbp_reset(self.h))

    def set_directions(self, mat_g, threshold, diameter=None):
        """mat_g [no_mats, 4] = x, y, z, count; the absolute threshold (relative times the sum of the counts); diameter (default D)"""
        g = np.ascontiguousarray(np.asarray(mat_g, dtype=np.float64).reshape(-1, 4))
        check(lib().xh_wbp_set_directions(self.h, _np_ptr(g), len(g), float(threshold), int(self.D if diameter is None else diameter)))
        self.no_mats = len(g)

    def add(self, images, rows, filtered=False):
        """filters and back-projects the images in list order; filtered=True returns the filtered images float64 [n, D, D]"""
        images = np.ascontiguousarray(images, np.float32)
        rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, self.ROW))
        if images.shape != (len(rows), self.D, self.D):
            raise XhError(f"ReconstructWbp: images of shape {images.shape} for {len(rows)} rows, the handle D = {self.D}")
        out = np.zeros(images.shape) if filtered else None
        check(lib().xh_wbp_add(self.h, _np_ptr(images), _np_ptr(rows), len(rows), _np_ptr(out)))
        return out

    def finish(self, R=None):
        """with the R of SymList::getMatrices [n, 3, 3]: symmetrizeVolume at its defaults, then the inner sphere of the diameter"""
        R = np.zeros((0, 3, 3)) if R is None else np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(-1, 3, 3))
        check(lib().xh_wbp_finish(self.h, _np_ptr(R) if len(R) else None, len(R)))

    def volume(self):
        """the volume as a float64 device tensor [D, D, D]"""
        out = self._new()
        check(lib().xh_wbp_volume(self.h, _ptr(out)))
        return out

    def count_thr(self):
        """Fourier pixels for which the threshold was not reached, over the images added since reset"""
        c = C.c_int64()
        check(lib().xh_wbp_count_thr(self.h, C.byref(c)))
        return c.value

    def weights(self, row):
        """the filter's weights of one image's row, [D, D] with the logical origin at (D // 2, D // 2) as after CenterFFT (test hook)"""
        row = np.ascontiguousarray(np.asarray(row, dtype=np.float64).reshape(self.ROW))
        w = np.zeros((self.D, self.D))
        check(lib().xh_wbp_weights(self.h, _np_ptr(row), _np_ptr(w)))
        return np.roll(w, (self.D // 2, self.D // 2), axis=(0, 1))

    def table(self):
        """the sinc table Tabsinc(0.0001, D) (test hook)"""
        n = C.c_int64()
        check(lib().xh_wbp_table(self.h, None, C.byref(n)))
        t = np.zeros(n.value)
        check(lib().xh_wbp_table(self.h, _np_ptr(t), C.byref(n)))
        return t


def wbp_image_matrices(rot, tilt, psi):
    """(row 2 of Euler_angles2matrix(rot, -tilt, psi), Euler_angles2matrix(-rot, tilt, -psi), inv(Euler_angles2matrix(rot, -tilt, psi))) (host only)"""
    g, F, B = np.zeros(3), np.zeros((3, 3)), np.zeros((3, 3))
    check(lib().xh_wbp_image_matrices(float(rot), float(tilt), float(psi), _np_ptr(g), _np_ptr(F), _np_ptr(B)))
    return g, F, B


def wbp_even_distribution(sampling):
    """make_even_distribution without symmetry, mirrors included: (rot [n], tilt [n]) in degrees (host only)"""
    n = C.c_int32()
    check(lib().xh_wbp_even_distribution(float(sampling), None, None, 0, C.byref(n)))
    rot, tilt = np.zeros(n.value), np.zeros(n.value)
    check(lib().xh_wbp_even_distribution(float(sampling), _np_ptr(rot), _np_ptr(tilt), n.value, C.byref(n)))
    return rot, tilt


def wbp_nearest_direction(rot, tilt, rot_list, tilt_list):
    """find_nearest_direction without symmetry: the index into the lists, -1 for empty lists (host only)"""
    r, t = np.ascontiguousarray(rot_list, np.float64), np.ascontiguousarray(tilt_list, np.float64)
    i = C.c_int32()
    check(lib().xh_wbp_nearest_direction(float(rot), float(tilt), _np_ptr(r), _np_ptr(t), len(r), C.byref(i)))
    return i.value


def wbp_tile():
    """the directions of one LDS tile of the filter kernel (host only)"""
    return lib().xh_wbp_tile()


class PsdEstimator(_StageTimes, _Handle):
    """The device side of the PSD stage of xmipp_ctf_estimate_from_micrograph (dtype float64: statisticsAdjust, normalize_ramp, the
    taper, |F|^2 pieceDim^2, avg and std) and of xmipp_psd_estimate (dtype float32: statisticsAdjust, the taper, the sum of the
    magnitudes). One micrograph [Y, X] lives on the device as float32; pieces are [n, 2] top-left corners (row, column), `capacity` of
    them run at a time and no result depends on it."""

    _destroy = "xh_psd_destroy"
    _PREFIX = "psd"

    STAGES = ("statistics", "rows", "columns", "finish")
    ADJUST, RAMP = 1, 2

    def __init__(self, ctx, Y, X, py, px=None, capacity=64, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise XhError(f"PsdEstimator: dtype {self.dtype} (float32 or float64)")
        self.Y, self.X, self.py, self.px, self.capacity = int(Y), int(X), int(py), int(py if px is None else px), int(capacity)
        self.flags = self.ADJUST | (self.RAMP if self.dtype == np.float64 else 0)
        h = C.c_void_p()
        check(lib().xh_psd_create(ctx.h, self.Y, self.X, self.py, self.px, self.capacity, int(self.dtype == np.float64), C.byref(h)))
        super().__init__(ctx, h)

    def _corners(self, corners):
        c = np.ascontiguousarray(np.asarray(corners, dtype=np.int32).reshape(-1, 2))
        return c

    def load(self, micrograph):
        """a float32 [Y, X] numpy array, or a torch tensor (device, or page-locked host memory)"""
        if isinstance(micrograph, np.ndarray):
            m = np.ascontiguousarray(micrograph, np.float32)
            if m.shape != (self.Y, self.X):
                raise XhError(f"PsdEstimator: a micrograph of shape {m.shape}, the handle {(self.Y, self.X)}")
            check(lib().xh_psd_load(self.h, _np_ptr(m)))
            return
        t = micrograph
        if tuple(t.shape) != (self.Y, self.X) or t.dtype != _torch().float32 or not t.is_contiguous():
            raise XhError(f"PsdEstimator: the micrograph must be a contiguous float32 tensor of shape {(self.Y, self.X)}")
        check(lib().xh_psd_load(self.h, C.c_void_p(t.data_ptr())))

    def add(self, corners, stack=False, flags=None):
        """adds the pieces' PSDs to the running sums in list order; stack=True returns each piece's own PSD [n, py, px] instead"""
        c = self._corners(corners)
        out = np.zeros((len(c), self.py, self.px), self.dtype) if stack else None
        check(lib().xh_psd_add(self.h, _np_ptr(c), len(c), self.flags if flags is None else int(flags), _np_ptr(out)))
        return out

    def result(self):
        """(avg, std, n) in float64; (the sum of the magnitudes, zeros, n) in float32; [py, px], mirrored to the whole plane"""
        avg, std = np.zeros((self.py, self.px), self.dtype), np.zeros((self.py, self.px), self.dtype)
        n = C.c_int64()
        check(lib().xh_psd_result(self.h, _np_ptr(avg), _np_ptr(std), C.byref(n)))
        return avg, std, n.value

    def reset(self):
        """zero sums and zero pieces; the micrograph stays"""
        check(lib().xh_psd_reset(self.h))

    def smoother(self):
        """the taper [py, px] as the kernels form it (test hook)"""
        out = np.zeros((self.py, self.px), self.dtype)
        check(lib().xh_psd_smoother(self.h, _np_ptr(out)))
        return out

    def piece(self, corners, flags=None):
        """the prepared pieces [n, py, px] before the transform (test hook)"""
        c = self._corners(corners)
        out = np.zeros((len(c), self.py, self.px), self.dtype)
        check(lib().xh_psd_piece(self.h, _np_ptr(c), len(c), self.flags if flags is None else int(flags), _np_ptr(out)))
        return out


def psd_pieces(Y, X, pieceDim, overlap=0.5, skipBorders=2, mode="micrograph", pos=None):
    """the piece list of xmipp_ctf_estimate_from_micrograph: (corners [n, 2] = row, column; slots [n], the reference's 1-based N;
    div_Number). mode: micrograph, regions or particles (pos [n, 2] = x, y of the centres) (host only)"""
    m = {"micrograph": 0, "regions": 1, "particles": 2}[mode]
    p = None if pos is None else np.ascontiguousarray(np.asarray(pos, dtype=np.int64).reshape(-1, 2))
    n, div = C.c_int32(), C.c_int32()
    args = (int(Y), int(X), int(pieceDim), float(overlap), int(skipBorders), m, _np_ptr(p), 0 if p is None else len(p))
    check(lib().xh_psd_pieces(*args, None, None, 0, C.byref(n), C.byref(div)))
    corners, slots = np.zeros((n.value, 2), np.int32), np.zeros(n.value, np.int32)
    check(lib().xh_psd_pieces(*args, _np_ptr(corners), _np_ptr(slots), n.value, C.byref(n), C.byref(div)))
    return corners, slots, div.value


def psd_patches(Y, X, py, px, borderX=0, borderY=0, overlap=0.5):
    """getPatchesLocation of xmipp_psd_estimate: corners [n, 2] = row, column (host only)"""
    n = C.c_int32()
    args = (int(Y), int(X), int(py), int(px), int(borderX), int(borderY), float(overlap))
    check(lib().xh_psd_patches(*args, None, 0, C.byref(n)))
    corners = np.zeros((n.value, 2), np.int32)
    check(lib().xh_psd_patches(*args, _np_ptr(corners), n.value, C.byref(n)))
    return corners


def psd_strip():
    """the half-spectrum columns one workgroup of the column pass owns (host only)"""
    return lib().xh_psd_strip()


def vds_normalize_robust(v, clip=1.3284):
    """normalize_Robust of a float64 array with a zero background mask; returns a new array (host only)"""
    out = np.ascontiguousarray(v, np.float64).copy()
    check(lib().xh_vds_normalize_robust(_np_ptr(out), out.size, float(clip)))
    return out


class VolumeDeformSph(_Handle):
    """The device side of xmipp_volume_deform_sph: the Zernike3D deformation of degrees (L1, L2) that fits an input volume to a
    reference. Volumes are numpy float64 [Z, Y, X] on the host (they stay on the device once set); the variables x are
    [3 * nterms]: cx, then cy, then cz."""

    _destroy = "xh_vds_destroy"

    def __init__(self, ctx, shape, L1=3, L2=2, Rmax=-1.0, lam=0.00025):
        self.shape = tuple(int(s) for s in shape)
        assert len(self.shape) == 3
        self.L1, self.L2 = int(L1), int(L2)
        h = C.c_void_p()
        check(lib().xh_vds_create(ctx.h, *self.shape, self.L1, self.L2, float(Rmax), float(lam), C.byref(h)))
        super().__init__(ctx, h)
        r, n = C.c_double(), C.c_int32()
        check(lib().xh_vds_info(self.h, C.byref(r), C.byref(n), None))
        self.Rmax, self.nterms = r.value, n.value

    def _vols(self, v, lead=()):
        v = np.ascontiguousarray(v, np.float64)
        assert tuple(v.shape) == tuple(lead) + self.shape, v.shape
        return v

    def _x(self, x):
        x = np.ascontiguousarray(x, np.float64)
        assert x.shape == (3 * self.nterms,), x.shape
        return x

    def gauss(self, v, sigma):
        """the REALGAUSSIAN low pass exp(-pi^2 w^2 sigma^2) of a volume"""
        v = self._vols(v)
        out = np.empty_like(v)
        check(lib().xh_vds_gauss(self.h, float(sigma), _np_ptr(v), _np_ptr(out)))
        return out

    def set_pairs(self, I, R):
        """the (input, reference) pairs [npairs, Z, Y, X], already normalised"""
        I = np.ascontiguousarray(I, np.float64)
        I = self._vols(I, (I.shape[0],))
        R = self._vols(R, (I.shape[0],))
        check(lib().xh_vds_set_pairs(self.h, I.shape[0], _np_ptr(I), _np_ptr(R)))

    @property
    def sumVI(self):
        s = C.c_double()
        check(lib().xh_vds_info(self.h, None, None, C.byref(s)))
        return s.value

    def cost(self, x):
        """(cost, diff2, sumVD, modg) at x, float64 [4]"""
        out = np.zeros(4)
        check(lib().xh_vds_cost(self.h, _np_ptr(self._x(x)), _np_ptr(out)))
        return out

    def refine_stage(self, stage, x):
        """one stage of the search from x: (x, cost, iterations, evaluations)"""
        x = self._x(x).copy()
        fret, it, ev = C.c_double(), C.c_int32(), C.c_int64()
        check(lib().xh_vds_refine_stage(self.h, int(stage), _np_ptr(x), C.byref(fret), C.byref(it), C.byref(ev)))
        return x, fret.value, it.value, ev.value

    def refine(self, x=None):
        """the program's loop, stages 0 .. L2: (x, cost, total evaluations)"""
        x = np.zeros(3 * self.nterms) if x is None else self._x(x)
        cost, evals = None, 0
        for stage in range(self.L2 + 1):
            x, cost, _, ev = self.refine_stage(stage, x)
            evals += ev
        return x, cost, evals

    def apply(self, raw, x, field=False):
        """raw sampled at the displaced positions; with field, also g [3, Z, Y, X]"""
        raw = self._vols(raw)
        VO = np.empty_like(raw)
        G = np.empty((3,) + self.shape) if field else None
        check(lib().xh_vds_apply(self.h, _np_ptr(raw), _np_ptr(self._x(x)), _np_ptr(VO), _np_ptr(G)))
        return (VO, G) if field else VO

    def strain(self, G):
        """(the field low-passed at sigma 2, local strain, local rotation in degrees) of a field [3, Z, Y, X]"""
        G = self._vols(G, (3,)).copy()
        LS, LR = np.empty(self.shape), np.empty(self.shape)
        check(lib().xh_vds_strain(self.h, _np_ptr(G), _np_ptr(LS), _np_ptr(LR)))
        return G, LS, LR


def powell_minimize(f, p, steps=None, ftol=0.01):
    """Powell's method of xmipp3_amd/host/powell.h (host only): f(x) takes the list of variables; returns (p, fmin, iterations)"""
    from ._lib import COST_FN
    p = np.ascontiguousarray(p, np.float64).copy()
    n = p.shape[0]
    steps = np.ones(n) if steps is None else np.ascontiguousarray(steps, np.float64)

    def cb(x, _user):
        return float(f([x[i + 1] for i in range(n)]))
    cfn = COST_FN(cb)
    fret, it = C.c_double(), C.c_int32()
    check(lib().xh_powell_minimize(n, _np_ptr(p), _np_ptr(steps), float(ftol), cfn, None, C.byref(fret), C.byref(it)))
    return p, fret.value, it.value


def powell_minimize_batch(f, problems, steps=None, ftol=0.01, capacity=64):
    """Many Powell searches in lockstep (xh_powell_minimize_batch, host only). problems: a list of starting vectors (any mix of
    lengths); f(idx, X) takes the problem indices of the rows and the list of their variable lists and returns their costs, one call per
    step over at most `capacity` live searches. Returns (list of minima, costs, iterations, cost calls): problem by problem what
    powell_minimize returns for it alone."""
    from ._lib import BATCH_COST_FN
    nprob = len(problems)
    n = np.asarray([len(q) for q in problems], np.int32)
    nmax = max(1, int(n.max())) if nprob else 1
    p = np.zeros((nprob, nmax))
    st = np.ones((nprob, nmax))
    for q in range(nprob):
        p[q, :n[q]] = problems[q]
        if steps is not None:
            st[q, :n[q]] = steps[q]
    failure = []

    def cb(m, problem, x, cost, _user):
        try:
            idx = [problem[r] for r in range(m)]
            rows = [[x[r * nmax + j] for j in range(n[idx[r]])] for r in range(m)]
            out = f(idx, rows)
            for r in range(m):
                cost[r] = float(out[r])
            return 0
        except BaseException as e:      # an exception must not cross the C frames: end the run and raise it afterwards
            failure.append(e)
            return 1
    cfn = BATCH_COST_FN(cb)
    fret, it, ev = np.zeros(nprob), np.zeros(nprob, np.int32), np.zeros(nprob, np.int64)
    rc = lib().xh_powell_minimize_batch(nprob, _np_ptr(n), nmax, _np_ptr(p), _np_ptr(st), float(ftol), int(capacity), cfn, None, _np_ptr(fret),
                                        _np_ptr(it), _np_ptr(ev))
    if failure:
        raise failure[0]
    check(rc)
    return [p[q, :n[q]].copy() for q in range(nprob)], fret, it, ev


def movie_binned_size(Y, X, binning):
    """AProgMovieAlignmentCorrelation::getMovieSize (movie_alignment_correlation_base.cpp:356-370): float arithmetic, truncated"""
    f = np.float32
    return int(f(f(f(Y) / f(binning)) / f(2)) * f(2)), int(f(f(f(X) / f(binning)) / f(2)) * f(2))


def movie_frames_to_float(ctx, raw, out=None):
    """Frames as the detector stores them (int8, int16, uint16, uint8 or float32 tensor on the device, any shape) -> float32, the
    cast of Image<float>::read (xh_movie_frame_to_float): copy the counts to the device, convert there."""
    torch = _torch()
    modes = {torch.int8: 0, torch.int16: 1, torch.float32: 2, torch.uint16: 6, torch.uint8: 100}
    assert raw.is_cuda and raw.is_contiguous() and raw.dtype in modes
    if out is None:
        out = torch.empty(raw.shape, dtype=torch.float32, device=raw.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == raw.numel()
    check(lib().xh_movie_frame_to_float(ctx.h, C.c_void_p(raw.data_ptr()), modes[raw.dtype], raw.numel(), _ptr(out)))
    return out


def movie_bin_frame(fft_raw, fft_binned, frame, dark=None, gain=None):
    """--bin of the CUDA FlexAlign program: frame [Y, X] -> [Yb, Xb] by cropping its half spectrum (xh_movie_bin_frame)"""
    torch = _torch()
    assert frame.is_cuda and frame.dtype == torch.float32 and frame.is_contiguous() and tuple(frame.shape) == (fft_raw.ny, fft_raw.nx)
    out = torch.empty((fft_binned.ny, fft_binned.nx), device=frame.device)
    check(lib().xh_movie_bin_frame(fft_raw.ctx.h, fft_raw.h, fft_binned.h, _ptr(frame), _ptr(dark, torch.float32), _ptr(gain, torch.float32), fft_raw.ny, fft_raw.nx,
                                   _ptr(out), fft_binned.ny, fft_binned.nx))
    return out


def movie_dose_filter(fft, frame, pixel_size, acc_voltage, dose_start, dose_finish):
    """ProgMovieFilterDose on one frame ([Y, X] float32 on the device, in place); fft = Fft2D(ctx, Y, X)."""
    torch = _torch()
    assert frame.is_cuda and frame.dtype == torch.float32 and frame.is_contiguous() and tuple(frame.shape) == (fft.ny, fft.nx)
    check(lib().xh_movie_dose_filter(fft.ctx.h, fft.h, _ptr(frame), fft.ny, fft.nx, float(pixel_size), float(acc_voltage), float(dose_start), float(dose_finish)))
    return frame


def fa_correlate(ctx, frames, max_dist):
    """CUDAFlexAlignCorrelate::run: frames [N, Y, X] float32 on the device (even sizes) -> positions [N (N-1)/2, 2] (x, y) of the
    correlation maxima of all pairs i < j."""
    torch = _torch()
    assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous() and frames.dim() == 3
    N, Y, X = frames.shape
    pos = np.empty((N * (N - 1) // 2, 2))
    check(lib().xh_fa_correlate(ctx.h, _ptr(frames), N, Y, X, float(max_dist), _np_ptr(pos)))
    return pos


class CtfOps(_Handle):
    """CTF pre-steps on the device: actualPhaseFlip (reconstruction/ctf_phase_flip.cpp:88-117) and
    Wiener2D::applyWienerFilter (data/wiener2d.cpp:101-141) for images of one size."""

    _destroy = "xh_ctfop_destroy"

    def __init__(self, ctx, ydim, xdim, pad=1.0):
        self.ctx, self.ydim, self.xdim = ctx, int(ydim), int(xdim)
        h = C.c_void_p()
        check(lib().xh_ctfop_create(ctx.h, self.ydim, self.xdim, float(pad), C.byref(h)))
        super().__init__(ctx, h)

    def phase_flip(self, img, ctf, sampling_rate):
        """img: [ydim, xdim] float32 on the device, flipped in place"""
        torch = _torch()
        assert img.is_cuda and img.dtype == torch.float32 and img.is_contiguous() and tuple(img.shape) == (self.ydim, self.xdim)
        check(lib().xh_ctfop_phase_flip(self.h, _ptr(img), C.byref(ctf), float(sampling_rate)))
        return img

    def wiener2d(self, imgs, ctfs, sampling_rate=1.0, phase_flipped=False, is_isotropic=False, wiener_constant=-1.0, correct_envelope=False):
        """imgs: [n, ydim, xdim] float32 on the device, corrected in place; ctfs: list of CtfParams or ctf_param_array"""
        torch = _torch()
        n = imgs.shape[0]
        assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.is_contiguous() and tuple(imgs.shape[1:]) == (self.ydim, self.xdim)
        arr = ctfs if isinstance(ctfs, C.Array) else (CtfParams * n)(*ctfs)
        check(lib().xh_ctfop_wiener2d(self.h, _ptr(imgs), n, arr, float(sampling_rate), int(phase_flipped), int(is_isotropic),
                                      float(wiener_constant), int(correct_envelope)))
        return imgs


class FourierProjector(_Handle):
    """Device side of FourierProjector (data/fourier_projection.cpp): central-slice projections of a
    volume `[z][y][x]` (float32, cuda) with cubic B-spline interpolation in Fourier space."""

    _destroy = "xh_fp_destroy"

    def __init__(self, ctx, vol, padding=2.0, max_freq=0.5, degree=3):
        torch = _torch()
        assert vol.is_cuda and vol.dtype == torch.float32 and vol.is_contiguous() and vol.dim() == 3
        self.ctx = ctx
        self.D = vol.shape[0]
        h = C.c_void_p()
        check(lib().xh_fp_create(ctx.h, _ptr(vol), self.D, float(padding), float(max_freq), int(degree), C.byref(h)))
        super().__init__(ctx, h)
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().xh_fp_info(h, C.byref(a), C.byref(b), C.byref(c)))
        self.P, self.cdim, self.cstart = a.value, b.value, c.value

    def coefs(self):
        re = np.empty((self.cdim,) * 3, np.float64)
        im = np.empty((self.cdim,) * 3, np.float64)
        check(lib().xh_fp_coefs(self.h, _np_ptr(re), _np_ptr(im)))
        return re, im

    def project(self, angles, ctf=None):
        """angles: [n, 3] (rot, tilt, psi) in degrees; ctf: optional float64 cuda tensor [D, D//2+1]."""
        torch = _torch()
        ang = np.ascontiguousarray(angles, np.float64).reshape(-1, 3)
        n = ang.shape[0]
        out = torch.empty((n, self.D, self.D), dtype=torch.float32, device=self.ctx.torch_device)
        check(lib().xh_fp_project(self.h, _np_ptr(ang), n, None if ctf is None else _ptr(ctf, torch.float64), _ptr(out)))
        return out


class RealSpaceProjector(_Handle):
    """Device side of projectVolume in real space (data/projection.cpp:337-589): four rays per pixel through the voxel grid of a
    volume `[z][y][x]` (float64, cuda, Xmipp origin). mode "value": the line integrals; mode "support": 1.0 where the line integral
    of a non-negative volume is positive, from the volume's v > 0 packed into bits (`packed`; a volume with a negative voxel takes the
    value walk followed by > 0)."""

    _destroy = "xh_rsp_destroy"
    MODES = {"value": 0, "support": 1}

    def __init__(self, ctx, vol, mode="value"):
        torch = _torch()
        if mode not in self.MODES:
            raise XhError(f"RealSpaceProjector: mode {mode!r} is neither 'value' nor 'support'")
        if not (vol.is_cuda and vol.dtype == torch.float64 and vol.is_contiguous() and vol.dim() == 3
                and vol.shape[0] == vol.shape[1] == vol.shape[2]):
            raise XhError("RealSpaceProjector: the volume must be a contiguous cubic float64 cuda tensor")
        self.D, self.mode = vol.shape[0], mode
        h = C.c_void_p()
        check(lib().xh_rsp_create(ctx.h, _ptr(vol), self.D, self.MODES[mode], C.byref(h)))
        super().__init__(ctx, h)
        packed = C.c_int32()
        check(lib().xh_rsp_info(h, None, None, C.byref(packed)))
        self.packed = bool(packed.value)

    def _args(self, angles, offsets):
        ang = np.ascontiguousarray(angles, np.float64).reshape(-1, 3)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.float64).reshape(-1, 2)
        if off is not None and off.shape[0] != ang.shape[0]:
            raise XhError(f"RealSpaceProjector: {ang.shape[0]} orientations but {off.shape[0]} offsets")
        return ang, off

    def project(self, angles, offsets=None):
        """angles: [n, 3] (rot, tilt, psi) in degrees; offsets: optional [n, 2], the roffset (x, y). Returns [n, D, D] float64."""
        torch = _torch()
        ang, off = self._args(angles, offsets)
        out = torch.empty((ang.shape[0], self.D, self.D), dtype=torch.float64, device=self.ctx.torch_device)
        check(lib().xh_rsp_project(self.h, _np_ptr(ang), _np_ptr(off), ang.shape[0], _ptr(out)))
        return out

    def steps(self, angles, offsets=None):
        """The voxel steps the four rays of every pixel walk in this handle's mode: [n, D, D] int32."""
        torch = _torch()
        ang, off = self._args(angles, offsets)
        out = torch.empty((ang.shape[0], self.D, self.D), dtype=torch.int32, device=self.ctx.torch_device)
        check(lib().xh_rsp_steps(self.h, _np_ptr(ang), _np_ptr(off), ang.shape[0], _ptr(out)))
        return out


def sub_freq_map(D, sampling=1.0, max_resolution=-1.0):
    """Host only: xmipp_subtract_projection's integer frequency map wi [D, D//2+1] and maxwiIdx."""
    wi = np.empty((D, D // 2 + 1), np.int32)
    mx = C.c_int32()
    check(lib().xh_sub_freq_map(int(D), float(sampling), float(max_resolution), _np_ptr(wi), C.byref(mx)))
    return wi, mx.value


def sub_fit(sums, maxwi, a11):
    """Host only: beta00, beta01, beta1 from the per-wi sums [maxwi + 1, 4] (xh_sub_fit)."""
    s = np.ascontiguousarray(sums, np.float64)
    if s.shape != (maxwi + 1, 4):
        raise XhError(f"sub_fit: sums of shape {s.shape}, expected {(maxwi + 1, 4)}")
    out = np.empty(3)
    check(lib().xh_sub_fit(_np_ptr(s), int(maxwi), float(a11), _np_ptr(out)))
    return tuple(out)


def sub_choose(sumY, sumY2, sumE0, sumE1, cells):
    """Host only: checkBestModel on the sums of evaluateFitting: (R2adj, model, R20adj)."""
    out = np.empty(3)
    check(lib().xh_sub_choose(float(sumY), float(sumY2), float(sumE0), float(sumE1), float(cells), _np_ptr(out)))
    return out[0], int(out[1]), out[2]


class SubtractProjection(_StageTimes, _Handle):
    """Device side of xmipp_subtract_projection (reconstruction/subtract_projection.cpp). vol, roi (--mask_roi) and mask (--mask): host
    arrays [D, D, D]; params: sampling, max_resolution, padding, cirmaskrad, subtract, real_space, ignore_ctf, boost, non_negative."""

    _destroy = "xh_sub_destroy"

    def __init__(self, ctx, vol, roi=None, mask=None, capacity=64, **params):
        from ._lib import SubParams
        prm = SubParams()
        lib().xh_sub_defaults(C.byref(prm))
        for k, v in params.items():
            if k not in dict(SubParams._fields_) or k == "pad_":
                raise XhError(f"SubtractProjection: unknown parameter {k!r}")
            setattr(prm, k, type(getattr(prm, k))(v))
        vol = np.ascontiguousarray(vol, np.float64)
        if vol.ndim != 3 or not (vol.shape[0] == vol.shape[1] == vol.shape[2]):
            raise XhError(f"SubtractProjection: the volume must be cubic, got {vol.shape}")
        self.D = vol.shape[0]
        aux = []
        for name, a in (("roi", roi), ("mask", mask)):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64)
                if a.shape != vol.shape:
                    raise XhError(f"SubtractProjection: the {name} volume has shape {a.shape}, the volume {vol.shape}")
            aux.append(a)
        h = C.c_void_p()
        check(lib().xh_sub_create(ctx.h, _np_ptr(vol), self.D, _np_ptr(aux[0]), _np_ptr(aux[1]), C.byref(prm), int(capacity), C.byref(h)))
        super().__init__(ctx, h)
        a, b, c = C.c_int32(), C.c_int32(), C.c_double()
        check(lib().xh_sub_info(h, C.byref(a), C.byref(b), C.byref(c)))
        self.maxwi, self.padded, self.a11 = a.value, b.value, c.value
        self.n = 0

    def load(self, images, rows):
        """images [n, D, D] float32 (host); rows: dicts with rot, tilt, psi, shift_x, shift_y and optionally ctf (a CtfParams)."""
        from ._lib import SubRow
        img = np.ascontiguousarray(images, np.float32)
        n = img.shape[0]
        if len(rows) != n:
            raise XhError(f"SubtractProjection.load: {n} images but {len(rows)} rows")
        arr = (SubRow * n)()
        for r, q in zip(arr, rows):
            for k in ("rot", "tilt", "psi", "shift_x", "shift_y"):
                setattr(r, k, float(q.get(k, 0.0)))
            if q.get("ctf") is not None:
                r.has_ctf = 1
                r.ctf = q["ctf"]
        check(lib().xh_sub_load(self.h, _np_ptr(img), n, img.shape[1], img.shape[2], arr))
        self.n = n

    def run(self):
        """Returns Idiff [n, D, D] float64 and a list of dicts (R2adj, beta0, beta1, b, beta00, R20adj, model, disable, enabled)."""
        from ._lib import SubResult
        out = np.empty((self.n, self.D, self.D), np.float64)
        res = (SubResult * max(self.n, 1))()
        check(lib().xh_sub_run(self.h, _np_ptr(out), res))
        names = [f[0] for f in SubResult._fields_ if f[0] != "pad_"]
        return out, [{k: getattr(r, k) for k in names} for r in res[:self.n]]

    _PREFIX = "sub"
    STAGES = ("projection", "ctf", "masks", "prepare_spectra", "sums_fit", "models", "output")

    def last(self, index):
        """The planes of particle `index` of the last chunk (host arrays), its sums [maxwi + 1, 4] and its betas."""
        torch = _torch()
        planes = {k: torch.empty((self.D, self.D), dtype=torch.float64, device=self.ctx.torch_device) for k in ("P", "Pctf", "PmaskImg", "M", "iM", "Idiff")}
        sums = np.empty((self.maxwi + 1, 4))
        betas = np.empty(3)
        check(lib().xh_sub_last(self.h, int(index), *[_ptr(planes[k]) for k in ("P", "Pctf", "PmaskImg", "M", "iM", "Idiff")], _np_ptr(sums), _np_ptr(betas)))
        out = {k: v.cpu().numpy() for k, v in planes.items()}
        out["sums"], out["betas"] = sums, betas
        return out


class _LockstepRows(_Handle):
    """What the per-particle Powell programs share: load's rows, cost and stats. A subclass names its ABI prefix (_abi) and its row
    struct (_Row, with _row_defaults), and sets nvars before the first cost."""

    _row_defaults = {}

    def _fn(self, name):
        return getattr(lib(), f"xh_{self._abi}_{name}")

    def _load(self, images, rows):
        img = np.ascontiguousarray(images, np.float32)
        assert img.ndim == 3
        n = img.shape[0]
        arr = (self._Row * n)()
        for i in range(n):
            for k, v in self._row_defaults.items():
                setattr(arr[i], k, v)
            for k, v in (rows[i] if rows is not None else {}).items():
                if not hasattr(arr[i], k) or k == "has_ctf":
                    raise XhError(f"{type(self).__name__}.load: unknown column {k}")
                if k == "ctf":
                    if v is not None:
                        arr[i].ctf, arr[i].has_ctf = v, 1
                else:
                    setattr(arr[i], k, int(v) if k == "flip" else float(v))
        check(self._fn("load")(self.h, _np_ptr(img), n, img.shape[1], img.shape[2], arr))
        self.n = n

    def _cost(self, particles, variables):
        idx = np.ascontiguousarray(particles, np.int32).reshape(-1)
        x = np.ascontiguousarray(variables, np.float64).reshape(-1, self.nvars)
        assert x.shape[0] == idx.shape[0]
        out = np.zeros(idx.shape[0])
        check(self._fn("cost")(self.h, idx.shape[0], _np_ptr(idx), _np_ptr(x), _np_ptr(out)))
        return out

    def stats(self):
        s = np.zeros(4)
        check(self._fn("stats")(self.h, _np_ptr(s)))
        return {"steps": int(s[0]), "rows": int(s[1]), "device_s": s[2], "total_s": s[3]}


class ContinuousAssign2(_LockstepRows):
    """Device side of ProgAngularContinuousAssign2 (reconstruction/angular_continuous_assign2.cpp): Powell refinement of every
    particle's grey values, shift, scale and angles against projections of `vol` ([z][y][x] float32, cuda), all searches in lockstep.
    Keyword arguments are the fields of xh_ca2_params (the program's options); capacity = evaluations per device step."""

    _destroy = "xh_ca2_destroy"
    _abi, _Row, _row_defaults, nvars = "ca2", Ca2Row, {"gray_a": 1.0}, 13
    VARIABLES = ("a", "b", "shiftX", "shiftY", "scaleX", "scaleY", "scaleAngle", "rot", "tilt", "psi", "defocusU", "defocusV",
                 "defocusAngle")

    def __init__(self, ctx, vol, capacity=4096, **params):
        torch = _torch()
        assert vol.is_cuda and vol.dtype == torch.float32 and vol.is_contiguous() and vol.dim() == 3
        self.D = vol.shape[0]
        self.params = Ca2Params()
        lib().xh_ca2_defaults(C.byref(self.params))
        for k, v in params.items():
            if not hasattr(self.params, k):
                raise XhError(f"ContinuousAssign2: unknown parameter {k}")
            setattr(self.params, k, v)
        self.capacity = int(capacity)
        self.n = 0
        h = C.c_void_p()
        check(lib().xh_ca2_create(ctx.h, _ptr(vol), self.D, C.byref(self.params), self.capacity, C.byref(h)))
        super().__init__(ctx, h)

    def load(self, images, rows=None):
        """images: [n, D, D] float32 (host); rows: per particle a dict with any of rot, tilt, psi, shift_x, shift_y, flip, scale_x,
        scale_y, scale_angle, gray_a, gray_b, ctf (a CtfParams: the particle has a CTF) (defaults: 0, gray_a 1, no CTF)"""
        self._load(images, rows)

    def cost(self, particles, variables):
        """particles: [m] indices; variables: [m, 13] -> costs [m] (1e38 for a row out of bounds)"""
        return self._cost(particles, variables)

    def last_images(self, row=0):
        """(P, E, Ifilteredp) [D, D] float64 cuda tensors of one row of the last evaluation"""
        torch = _torch()
        out = [torch.empty((self.D, self.D), dtype=torch.float64, device=self.ctx.torch_device) for _ in range(3)]
        check(lib().xh_ca2_last_images(self.h, int(row), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return out

    def measures(self, row=0):
        """(corrIdx, corrMask, imed) between P and Ifilteredp of one row of the last evaluation"""
        out = np.zeros(3)
        check(lib().xh_ca2_measures(self.h, int(row), _np_ptr(out)))
        return tuple(out)

    def apply(self, images, variables):
        """the final transform of every loaded particle: images [n, D, D] float32 (host), variables [n, 13] -> [n, D, D] float32"""
        img = np.ascontiguousarray(images, np.float32)
        x = np.ascontiguousarray(variables, np.float64).reshape(-1, 13)
        assert img.shape == (self.n, self.D, self.D) and x.shape[0] == self.n
        out = np.empty_like(img)
        check(lib().xh_ca2_apply(self.h, _np_ptr(img), _np_ptr(x), _np_ptr(out)))
        return out

    def filtered(self, particle):
        """(Ifiltered [D, D] float64 numpy, Istddev) of a loaded particle"""
        out = np.empty((self.D, self.D))
        sd = C.c_double()
        check(lib().xh_ca2_filtered(self.h, int(particle), _np_ptr(out), C.byref(sd)))
        return out, sd.value

    def refine(self):
        """-> (variables [n, 13], cost [n], iterations [n], cost calls [n], enabled [n]) of every loaded particle"""
        n = self.n
        x, cost = np.zeros((n, 13)), np.zeros(n)
        it, ev, en = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
        check(lib().xh_ca2_refine(self.h, _np_ptr(x), _np_ptr(cost), _np_ptr(it), _np_ptr(ev), _np_ptr(en)))
        return x, cost, it, ev, en


def asa_stage_active(L1, L2, stage, deformation=True, alignment=False, defocus=False):
    """the indices of the variables that stage `stage` of xmipp_angular_sph_alignment frees, among the 3 vecSize + 8 of degrees (L1, L2)
    (host only)"""
    flags = (1 if deformation else 0) | (2 if alignment else 0) | (4 if defocus else 0)
    out = np.zeros(3 * 45 + 8, np.int32)
    n = C.c_int32()
    check(lib().xh_asa_stage_active(int(L1), int(L2), int(stage), flags, _np_ptr(out), C.byref(n)))
    return out[:n.value].copy()


class AngularSphAlignment(_LockstepRows):
    """Device side of ProgAngularSphAlignment (reconstruction/angular_sph_alignment.cpp): for every particle a pose and a Zernike3D
    deformation of `vol` ([z][y][x] float32, cuda, a cube), fitted by Powell's method, all searches in lockstep. mask: int32 [D, D, D]
    (numpy; None: the sphere of radius RDef). Keyword arguments are the fields of xh_asa_params (the program's options; lam is
    --regularization); capacity = evaluations per device step. The variables of a row are [3 vecSize + 8]: cx, cy, cz of every term,
    then the change of shift x, y, rot, tilt, psi, defocus U, V, defocus angle."""

    _destroy = "xh_asa_destroy"
    _abi, _Row = "asa", AsaRow
    POSE = ("shiftX", "shiftY", "rot", "tilt", "psi", "defocusU", "defocusV", "defocusAngle")

    def __init__(self, ctx, vol, mask=None, capacity=64, **params):
        torch = _torch()
        assert vol.is_cuda and vol.dtype == torch.float32 and vol.is_contiguous() and vol.dim() == 3
        if not (vol.shape[0] == vol.shape[1] == vol.shape[2]):
            raise XhError(f"AngularSphAlignment: the volume must be a cube, got {tuple(vol.shape)} (not supported)")
        self.D = vol.shape[0]
        self.params = AsaParams()
        lib().xh_asa_defaults(C.byref(self.params))
        for k, v in params.items():
            k = "lambda_" if k in ("lam", "lambda_") else k
            if not hasattr(self.params, k):
                raise XhError(f"AngularSphAlignment: unknown parameter {k}")
            setattr(self.params, k, v)
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.int32)
            if mask.shape != (self.D,) * 3:
                raise XhError(f"AngularSphAlignment: a mask of shape {mask.shape} against a volume of size {self.D} (not supported)")
        self.capacity = int(capacity)
        self.n = 0
        h = C.c_void_p()
        check(lib().xh_asa_create(ctx.h, _ptr(vol), self.D, _np_ptr(mask), C.byref(self.params), self.capacity, C.byref(h)))
        super().__init__(ctx, h)
        rd, rm, vs, nv, sv = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_double()
        check(lib().xh_asa_info(self.h, C.byref(rd), C.byref(rm), C.byref(vs), C.byref(nv), C.byref(sv)))
        self.RDef, self.Rmax, self.vecSize, self.nvars, self.sumV = rd.value, rm.value, vs.value, nv.value, sv.value

    def load(self, images, rows=None):
        """images: [n, D, D] float32 (host); rows: per particle a dict with any of rot, tilt, psi, shift_x, shift_y, flip, ctf (a
        CtfParams: the particle has a CTF) (defaults: 0, no CTF)"""
        self._load(images, rows)

    def cost(self, particles, variables):
        """particles: [m] indices; variables: [m, nvars] -> costs [m] (1e38 for a row out of bounds, and for one whose count is 0)"""
        return self._cost(particles, variables)

    def last(self, row=0):
        """(P_raw, P, Ifilteredp) [D, D] float64 cuda tensors and (sumVd, modg, count, corr) float64 [4] of one device row of the last
        evaluation"""
        torch = _torch()
        out = [torch.empty((self.D, self.D), dtype=torch.float64, device=self.ctx.torch_device) for _ in range(3)]
        sums = np.zeros(4)
        check(lib().xh_asa_last(self.h, int(row), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _np_ptr(sums)))
        return out[0], out[1], out[2], sums

    def refine(self):
        """-> (variables [n, nvars], cost [n], enabled [n], deformation [n], iterations [n], cost calls [n]) of every loaded particle"""
        n = self.n
        x, cost, de = np.zeros((n, self.nvars)), np.zeros(n), np.zeros(n)
        en, it, ev = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        check(lib().xh_asa_refine(self.h, _np_ptr(x), _np_ptr(cost), _np_ptr(en), _np_ptr(de), _np_ptr(it), _np_ptr(ev)))
        return x, cost, en, de, it, ev


def faz_sort_orthogonal(rot, tilt, sort_last=2):
    """the order in which xmipp_forward_art_zernike3d presents its images: every next direction has the smallest sum of |dot products| with
    the last `sort_last` ones presented (-1: with all of them); rot, tilt in degrees (host only)"""
    rot = np.ascontiguousarray(rot, np.float64).reshape(-1)
    tilt = np.ascontiguousarray(tilt, np.float64).reshape(-1)
    assert rot.shape == tilt.shape
    out = np.zeros(rot.shape[0], np.int32)
    check(lib().xh_faz_sort_orthogonal(rot.shape[0], _np_ptr(rot), _np_ptr(tilt), int(sort_last), _np_ptr(out)))
    return out


def faz_save_schedule(n, save_iter):
    """--save_iter over one iteration of n images: [n] flags, 1 where the partial volume is written after that image (host only)"""
    out = np.zeros(int(n), np.int32)
    check(lib().xh_faz_save_schedule(int(n), int(save_iter), _np_ptr(out)))
    return out


class ForwardArtZernike3D(_StageTimes, _Handle):
    """Device side of xmipp_forward_art_zernike3d: ART reconstruction of the undeformed volume of side D from particles with a pose and
    Zernike3D coefficients. volume: float64 [D, D, D] (numpy; None: zeros); maskf / maskb: int32 [D, D, D] (numpy; None: the sphere of
    radius RDef); sigma: the Gaussian sigmas; sym: [nsym, 3, 3] right matrices of the symmetry group without the identity. Keyword
    arguments are the fields of xh_faz_params (lam is --regularization). The volume stays on the device between calls."""

    _destroy = "xh_faz_destroy"

    def __init__(self, ctx, D, volume=None, maskf=None, maskb=None, sigma=(2.0,), sym=None, **params):
        self.D = int(D)
        self.params = FazParams()
        lib().xh_faz_defaults(C.byref(self.params))
        for k, v in params.items():
            k = "lambda_" if k in ("lam", "lambda_") else k
            if not hasattr(self.params, k):
                raise XhError(f"ForwardArtZernike3D: unknown parameter {k}")
            setattr(self.params, k, v)

        def vol(a, dtype, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype)
            if a.shape != (self.D,) * 3:
                raise XhError(f"ForwardArtZernike3D: {what} of shape {a.shape} against a volume of size {self.D} (not supported)")
            return a
        volume, maskf, maskb = vol(volume, np.float64, "a volume"), vol(maskf, np.int32, "a mask"), vol(maskb, np.int32, "a mask")
        sg = np.ascontiguousarray(sigma, np.float64).reshape(-1)
        s = None if sym is None else np.ascontiguousarray(sym, np.float64).reshape(-1, 9)
        self.nsigma = sg.shape[0]
        self.n = 0
        h = C.c_void_p()
        check(lib().xh_faz_create(ctx.h, self.D, _np_ptr(volume), _np_ptr(maskf), _np_ptr(maskb), _np_ptr(sg), self.nsigma, _np_ptr(s),
                                  0 if s is None else s.shape[0], C.byref(self.params), C.byref(h)))
        super().__init__(ctx, h)
        rd, vs, nb, per = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().xh_faz_info(self.h, C.byref(rd), C.byref(vs), C.byref(nb), C.byref(per)))
        self.RDef, self.vecSize, self.nbricks, self.per_image = rd.value, vs.value, nb.value, per.value

    def load(self, images, rows=None, coefficients=None):
        """images: [n, D, D] float32 (host); rows: per particle a dict with any of rot, tilt, psi, shift_x, shift_y, flip, ctf (a
        CtfParams); coefficients: [n, 3 vecSize] (cx of every term, then cy, then cz), needed with use_zernike"""
        img = np.ascontiguousarray(images, np.float32)
        assert img.ndim == 3
        n = img.shape[0]
        co = None
        if coefficients is not None:
            co = np.ascontiguousarray(coefficients, np.float64)
            if co.shape != (n, 3 * self.vecSize):
                raise XhError(f"ForwardArtZernike3D.load: coefficients of shape {co.shape}, the degrees need ({n}, {3 * self.vecSize})")
        arr = (FazRow * n)()
        for i in range(n):
            for k, v in (rows[i] if rows is not None else {}).items():
                if not hasattr(arr[i], k) or k == "has_ctf":
                    raise XhError(f"ForwardArtZernike3D.load: unknown column {k}")
                if k == "ctf":
                    if v is not None:
                        arr[i].ctf, arr[i].has_ctf = v, 1
                else:
                    setattr(arr[i], k, int(v) if k == "flip" else float(v))
        check(lib().xh_faz_load(self.h, _np_ptr(img), n, img.shape[1], img.shape[2], arr, _np_ptr(co)))
        self.n = n

    def sweep(self, first=0, count=None):
        """forward, residual, regulariser and update for the loaded images first .. first + count - 1 in order -> errors [count, per_image]"""
        count = self.n - first if count is None else int(count)
        err = np.zeros((count, self.per_image))
        check(lib().xh_faz_sweep(self.h, int(first), count, _np_ptr(err)))
        return err

    def forward(self, index, sym=0):
        """the forward model of one presentation against the current volume, which is not updated -> dict of float64 cuda tensors P_raw,
        W_raw, P, W [nsigma, D, D], Idiff, Iws, particle [D, D], and error"""
        torch = _torch()
        D, S = self.D, self.nsigma
        mk = lambda *shape: torch.empty(shape, dtype=torch.float64, device=self.ctx.torch_device)  # noqa: E731
        out = {"P_raw": mk(S, D, D), "W_raw": mk(S, D, D), "P": mk(S, D, D), "W": mk(S, D, D), "Idiff": mk(D, D), "Iws": mk(D, D),
               "particle": mk(D, D)}
        err = C.c_double()
        check(lib().xh_faz_forward(self.h, int(index), int(sym), *[_ptr(out[k]) for k in ("P_raw", "W_raw", "P", "W", "Idiff", "Iws", "particle")],
                                   C.byref(err)))
        out["error"] = err.value
        return out

    def get_volume(self):
        out = np.empty((self.D,) * 3)
        check(lib().xh_faz_get_volume(self.h, _np_ptr(out)))
        return out

    def set_volume(self, volume):
        v = np.ascontiguousarray(volume, np.float64)
        assert v.shape == (self.D,) * 3
        check(lib().xh_faz_set_volume(self.h, _np_ptr(v)))

    _PREFIX = "faz"
    STAGES = ("splat", "filter", "residual", "regulariser", "backward")      # of the last timed sweep, summed over its presentations


class ProjectionMatcher(_Handle):
    """Device side of ProgAngularProjectionMatching
    (reconstruction/angular_projection_matching.cpp)."""

    _destroy = "xh_pm_destroy"

    def __init__(self, ctx, refs, Ri=1, Ro=-1, Mctf=None, paddim=0):
        torch = _torch()
        assert refs.is_cuda and refs.dtype == torch.float32 and refs.is_contiguous()
        self.ctx = ctx
        self.nrefs, self.D, _ = refs.shape
        h = C.c_void_p()
        m = None if Mctf is None else np.ascontiguousarray(Mctf, np.float64)
        check(lib().xh_pm_create(ctx.h, self.D, Ri, Ro, self.nrefs, _ptr(refs), _np_ptr(m), paddim, C.byref(h)))
        super().__init__(ctx, h)
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        check(lib().xh_pm_info(h, C.byref(a), C.byref(b), C.byref(c)))
        self.N, self.ncoef, self.nsamples = a.value, b.value, c.value

    def set_option(self, name, value):
        check(lib().xh_pm_set_option(self.h, name.encode(), float(value)))

    def match(self, particles, nbr_off=None, nbr_ids=None, parity=0, n_orient=1, shifts5d=None):
        """Rotational search (APM:530-760). shifts5d: (xoff[], yoff[]) integer 5-D search translations
        (`search5d_offsets`); n_orient > 1 returns [n, n_orient] arrays (refno -1 = rank not filled)."""
        torch = _torch()
        assert particles.is_cuda and particles.dtype == torch.float32 and particles.is_contiguous()
        n = particles.shape[0]
        dev = particles.device
        shape = (n,) if n_orient == 1 else (n, n_orient)
        refno = torch.empty(shape, dtype=torch.int32, device=dev)
        psi = torch.empty(shape, dtype=torch.int32, device=dev)
        flip = torch.empty(shape, dtype=torch.uint8, device=dev)
        off = ids = xo = yo = None
        nt = 0
        if nbr_off is not None:
            off = np.ascontiguousarray(nbr_off, np.int32)
            ids = np.ascontiguousarray(nbr_ids, np.int32)
        if shifts5d is not None:
            xo = np.ascontiguousarray(shifts5d[0], np.int32)
            yo = np.ascontiguousarray(shifts5d[1], np.int32)
            nt = len(xo)
            assert len(yo) == nt and nt > 0
        check(lib().xh_pm_match_ex(self.h, _ptr(particles), n, _np_ptr(off), _np_ptr(ids), int(parity), int(n_orient), nt,
                                   _np_ptr(xo), _np_ptr(yo), _ptr(refno), _ptr(psi), _ptr(flip)))
        return refno, psi, flip

    def translate(self, particles, refno, psi, flip, max_shift=-1.0):
        torch = _torch()
        n = particles.shape[0]
        dev = particles.device
        sx = torch.empty(n, dtype=torch.float64, device=dev)
        sy = torch.empty_like(sx)
        cc = torch.empty_like(sx)
        check(lib().xh_pm_translate(self.h, _ptr(particles, torch.float32), n, _ptr(refno, torch.int32), _ptr(psi, torch.int32),
                                    _ptr(flip, torch.uint8), float(max_shift),
                                    _ptr(sx), _ptr(sy), _ptr(cc)))
        return sx, sy, cc

    def translate_repeated(self):
        """Particles the last translate() repeated in double precision (its first pass is fp32)."""
        r = C.c_int64()
        check(lib().xh_pm_translate_stats(self.h, C.byref(r)))
        return r.value

    def stage_ms(self, reset=True):
        ms = np.zeros(8, np.float64)
        check(lib().xh_pm_stage_ms(self.h, _np_ptr(ms), int(reset)))
        return dict(zip(("prep32", "contract", "idft_max", "select", "rescore_fp64"), ms[:5].tolist()))

    def two_level_cut(self):
        """(K0, nk): the contraction of the dense search stops at angular frequency K0 (xh_pm_two_level_cut)."""
        a, b = C.c_int32(), C.c_int32()
        check(lib().xh_pm_two_level_cut(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_coefficients(self, n):
        """Device pointer to the fp32 B-spline coefficients of the n particles of the last match() call, or None when
        that call ran in several chunks (or with the recursive prefilter): valid until the next call on this matcher."""
        p, a, b = C.c_void_p(), C.c_int32(), C.c_int32()
        check(lib().xh_pm_last_coefficients(self.h, C.byref(p), C.byref(a), C.byref(b)))
        return p.value if (p.value and a.value == 0 and b.value == n) else None

    def last_stats(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().xh_pm_last_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        d = C.c_int64()
        check(lib().xh_pm_rows_pruned(self.h, C.byref(d)))
        return {"rows": a.value, "rescored_particles": b.value, "rescored_rows": c.value, "pruned_rows": d.value}

    # ---- test hooks
    def debug_prepare(self, particles, precision=32):
        n = particles.shape[0]
        coefs = np.empty((n, self.ncoef, 2), np.float64)
        sigma = np.empty(n, np.float64)
        check(lib().xh_pm_debug_prepare(self.h, _ptr(particles), n, precision, _np_ptr(coefs), _np_ptr(sigma)))
        return coefs[..., 0] + 1j * coefs[..., 1], sigma

    def debug_ref(self, r):
        coefs = np.empty((self.ncoef, 2), np.float64)
        s = C.c_double()
        check(lib().xh_pm_debug_ref(self.h, r, _np_ptr(coefs), C.byref(s)))
        return coefs[:, 0] + 1j * coefs[:, 1], s.value

    def debug_corr_rows(self, particle, ref, precision=32):
        out = np.empty(2 * self.N, np.float64)
        check(lib().xh_pm_debug_corr_rows(self.h, _ptr(particle), ref, precision, _np_ptr(out)))
        return out

    def debug_s6_maps(self, n):
        """correlation maps left by the last translate() under set_option("s6_capture", 32 | 64): [n, D, D] float64"""
        out = np.empty((n, self.D, self.D), np.float64)
        check(lib().xh_pm_debug_s6_maps(self.h, n, _np_ptr(out)))
        return out

    def get_option(self, name):
        v = C.c_double()
        check(lib().xh_pm_get_option(self.h, name.encode(), C.byref(v)))
        return v.value
