"""Thin Python handle on a uwspr_ctx (include/uwspr_hip.h) for tests and bench.

Arrays in, arrays out; every number comes from the HIP library.  Frames may be
numpy arrays (host path: staged by the library) or torch CUDA tensors (device
path: pointers are passed through untouched).
"""
import ctypes as C

import numpy as np

from . import native as N

AUDIO_RATE = 12000
BLANK_BLOCK = 4096   # UWSPR_BLANK_BLOCK: samples per block of the blanker's level
FRONTEND_GRC, FRONTEND_COMPACT = 0, 1


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _ptr(x):
    """the data pointer of a numpy array or a torch tensor"""
    return C.c_void_p(x.data_ptr() if _is_torch(x) else x.ctypes.data)


def _empty(like, shape, dtype):
    """an uninitialised array of a numpy dtype where `like` lives: numpy, or a tensor on the tensor's device"""
    if _is_torch(like):
        import torch
        return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), device=like.device)
    return np.empty(tuple(shape), dtype)


def _audio_format(x):
    """AUDIO_F32 / AUDIO_S16 for a float32 / int16 numpy array or torch tensor, None for any other type"""
    if _is_torch(x):
        import torch
        return {torch.float32: N.AUDIO_F32, torch.int16: N.AUDIO_S16}.get(x.dtype)
    return {np.dtype(np.float32): N.AUDIO_F32, np.dtype(np.int16): N.AUDIO_S16}.get(x.dtype)


def _audio_block(x, who):
    """`who`'s audio: [n] or [n, C], float32 or int16, a numpy array (made contiguous) or a contiguous torch CUDA tensor
    -> (x, format, C)"""
    if _is_torch(x):
        if _audio_format(x) is None or x.dim() not in (1, 2) or not x.is_cuda or not x.is_contiguous() or x.shape[0] < 1:
            raise TypeError("%s: a contiguous [n] or [n, C] float32 or int16 CUDA tensor, not %s %s" % (who, x.dtype, tuple(x.shape)))
    else:
        x = np.asarray(x)
        if x.ndim not in (1, 2) or _audio_format(x) is None or x.shape[0] < 1:
            raise TypeError("%s: a [n] or [n, C] float32 or int16 array, not %s %s" % (who, x.dtype, x.shape))
        x = np.ascontiguousarray(x)
    return x, _audio_format(x), 1 if len(x.shape) == 1 else x.shape[1]


def _audio_array(x):
    """a 1-D contiguous float32 or int16 numpy array, as it is (no conversion: the library reads both)"""
    a = np.asarray(x)
    if a.ndim != 1 or a.dtype not in (np.float32, np.int16):
        raise TypeError("audio: a 1-D float32 or int16 array, not %s %s" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def _launch_tensors(who, audio, out=None):
    """what the debug_*_launch methods check of their tensors (the library sees pointers only) -> audio's format"""
    import torch
    fmt = _audio_format(audio)
    if fmt is None or not audio.is_cuda or not audio.is_contiguous():
        raise TypeError("%s: a contiguous float32 or int16 CUDA tensor, not %s" % (who, audio.dtype))
    if out is not None and (out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous()):
        raise TypeError("%s: out is a contiguous float32 CUDA tensor, not %s" % (who, out.dtype))
    return fmt


def _tx_call(L, kind, h, sig, mot, car, fad, imp, *rest):
    """One uwspr_tx_<kind>* call, kind "baseband" or "render", routed by what the transmissions carry (the arrays of
    tx_motions, tx_carriers, tx_fades, tx_impulses, or None): _medium with any fading or impulses, else _at with any
    carrier, else _moving with any motion, else the plain entry.  A route's arrays follow `signals`; render_medium's
    impulses follow the channels (rest[1]).  `rest`: the arguments every route takes behind those."""
    sp = C.c_void_p(C.addressof(sig)) if len(sig) else None
    mp = None if mot is None else C.c_void_p(C.addressof(mot))
    cp = None if car is None else C.c_void_p(car.ctypes.data)
    if fad is not None or imp is not None:
        fp = None if fad is None else C.c_void_p(C.addressof(fad))
        if kind == "render":
            rest = rest[:2] + (None if imp is None else C.c_void_p(C.addressof(imp)),) + rest[2:]
        return getattr(L, "uwspr_tx_%s_medium" % kind)(h, sp, mp, cp, fp, *rest)
    if car is not None:
        return getattr(L, "uwspr_tx_%s_at" % kind)(h, sp, mp, cp, *rest)
    if mot is not None:
        return getattr(L, "uwspr_tx_%s_moving" % kind)(h, sp, mp, *rest)
    return getattr(L, "uwspr_tx_" + kind)(h, sp, *rest)


def _cand_lists(cands, npk):
    """the (cands, npk) buffers of Context._cand_buffers after the call -> per frame, its candidate records"""
    if _is_torch(cands):
        cands = np.frombuffer(cands.cpu().numpy().tobytes(), N.CAND_DTYPE).reshape(npk.numel(), -1)
        npk = npk.cpu().numpy()
    return [cands[b, :npk[b]].copy() for b in range(len(npk))]


class FrameView:
    """B frames that are not a contiguous [B, fl, 2] array: either a raw device pointer (what
    stream_take_view returns: frames in place in the stream buffer) or a host array holding a stretch
    of the stream.  Frame b starts at 2*stride*b floats; pair with Context.set_frame_stride(stride)."""

    def __init__(self, B, ptr=None, host=None, device=0):
        self.B = int(B)
        self.ptr = ptr
        self.host = None if host is None else np.ascontiguousarray(host, dtype=np.float32)
        self._dev = device

    @property
    def device(self):
        import torch
        return torch.device("cuda", self._dev)


class Context:
    """Parameters mirror gr::uwspr::FDR::make / sync_and_demodulate::make
    (include/uwspr/FDR.h:49-50, include/uwspr/sync_and_demodulate.h:49)."""

    def __init__(self, fs=375, fl=45000, spb=256, maxdrift=0, maxfreqs=200, halfbandwidth=10,
                 cf=1500, threshold=10, device=0, options=None):
        """options: {name: int} for uwspr_set_option ("sched", "stage_kernels", "reuse", "phasor_tables",
        "fast_search", ...: include/uwspr_hip.h)."""
        self.L = N.lib()
        self.params = N.Params(fs, fl, spb, maxdrift, maxfreqs, halfbandwidth, cf, threshold)
        self.h = C.c_void_p()
        rc = self.L.uwspr_ctx_create(C.byref(self.params), device, C.byref(self.h))
        if rc != 0:
            msg = self.L.uwspr_last_error(self.h).decode() if self.h else \
                self.L.uwspr_status_string(rc).decode()
            if self.h:
                self.L.uwspr_ctx_destroy(self.h)
                self.h = C.c_void_p()
            raise N.UwsprError(rc, msg)
        self.info = N.Info()
        self._chk(self.L.uwspr_get_info(self.h, C.byref(self.info)))
        self.fl, self.maxfreqs = fl, maxfreqs
        self._stream_ptr = None
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name, value):
        self._chk(self.L.uwspr_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int32()
        self._chk(self.L.uwspr_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def close(self):
        if getattr(self, "h", None):
            self.L.uwspr_ctx_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise N.UwsprError(rc, self.L.uwspr_last_error(self.h).decode())

    # -- helpers -----------------------------------------------------------
    def _frames(self, frames):
        """-> (pointer, B, where, keepalive)"""
        if isinstance(frames, FrameView):      # B frames at a raw pointer, pitch per set_frame_stride
            if frames.host is not None:
                return C.c_void_p(frames.host.ctypes.data), frames.B, N.HOST, frames.host
            return C.c_void_p(frames.ptr), frames.B, N.DEVICE, frames
        if _is_torch(frames):
            assert frames.is_cuda and frames.is_contiguous() and frames.dtype.is_floating_point
            assert frames.element_size() == 4
            B = frames.numel() // (2 * self.fl)
            if self._stream_ptr is None:   # (asked here as well: with a caller's stream the timed calls pay for nothing more)
                self._wait_torch(frames.device)
            return C.c_void_p(frames.data_ptr()), B, N.DEVICE, frames
        a = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, self.fl, 2)
        return C.c_void_p(a.ctypes.data), a.shape[0], N.HOST, a

    def _cand_buffers(self, B, device=None):
        """(cands, npk) for B frames' candidates: numpy arrays, or for a torch device byte / int32 tensors there"""
        if device is None:
            return np.zeros((B, self.maxfreqs), N.CAND_DTYPE), np.zeros(B, np.int32)
        import torch
        return (torch.empty(B * self.maxfreqs * 48, dtype=torch.uint8, device=device),
                torch.empty(B, dtype=torch.int32, device=device))

    def set_stream(self, stream_ptr):
        """Run on a caller's hipStream_t (e.g. torch.cuda.Stream().cuda_stream); the caller
        then owns the ordering against its own work on that stream.  None/0 = own stream."""
        self._chk(self.L.uwspr_set_stream(self.h, C.c_void_p(stream_ptr)))
        self._stream_ptr = stream_ptr or None

    def synchronize(self):
        self._chk(self.L.uwspr_synchronize(self.h))

    # -- the door between torch's stream and the context's (DESIGN.md lists each method's variant) ----
    def _wait_torch(self, device, always=False):
        """Before a call on device tensors: the library runs on the context's own stream, so whatever torch queued on its
        current stream of `device` (None: the current device) to produce them must have finished first -- unless the
        caller set a stream and so owns the ordering, and the call site does not say `always`."""
        if self._stream_ptr is None or always:
            import torch
            torch.cuda.current_stream(device).synchronize()

    def _wait_self(self, always):
        """After a call that left results on the device: synchronize the context -- always (the method reads them on the
        host next), or (always=False) only when the context runs on its own stream, a caller's stream being the
        caller's to wait for."""
        if self._stream_ptr is None or always:
            self.synchronize()

    def debug_snr_db(self, x):
        """diagnostics: 10 * log10f(x) as K2 computes a candidate's `snr` (FDR_impl.cc:303); x, result: float32 CUDA tensors"""
        import torch
        out = torch.empty_like(x)
        self._wait_torch(None, always=True)
        self._chk(self.L.uwspr_debug_snr_db(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel()))
        self._wait_self(always=True)
        return out

    LAUNCH_FORMS = ("flat_t1", "flat_t2", "flat_t4", "flat_fast", "fold_wave", "fold_lanes",
                    "grid_nl1", "grid_nl2", "grid_nl4", "grid_nl5", "grid_nl6", "grid_nl8",
                    "grid_wpw1", "grid_wpw2", "grid_wpw4", "grid_fallback",
                    "fold_wave_soft", "fold_lanes_soft", "fold_wave_pwin", "fold_lanes_pwin")

    def launch_forms(self):
        """diagnostics: launches of the sweep kernels per form since the context was created (uwspr_debug_launch_forms:
        host-side counters of launch_tonecorr, launch_fold, launch_grid_block and the fallback of uwspr_sync_grid) ->
        {name: count}: the flat kernel by tones per lane, the fold by form (and, of those, the launches with soft
        symbols and with the stage winner's magnitudes), the grid kernel by lags per block and by wavefronts per
        workgroup, and the grid calls that fell back to the flat kernel."""
        out = np.zeros(len(self.LAUNCH_FORMS), np.int64)
        n = self.L.uwspr_debug_launch_forms(self.h, C.c_void_p(out.ctypes.data), out.size)
        if n != out.size:
            raise N.UwsprError(n if n < 0 else -1, "uwspr_debug_launch_forms: %d slots, this binding names %d" % (n, out.size))
        return {k: int(v) for k, v in zip(self.LAUNCH_FORMS, out)}

    # -- front-end ---------------------------------------------------------
    def frontend(self, audio):
        """12 kS/s real audio [B, nin] -> frames [B, fl, 2] at 375 S/s (uwspr_frontend_batch)."""
        dev = _is_torch(audio)
        a = audio if dev else np.ascontiguousarray(audio, dtype=np.float32)
        a = a.reshape(1, -1) if not dev and a.ndim == 1 else a
        B, nin = a.shape
        out = _empty(a, (B, self.fl, 2), np.float32)
        if dev:
            self._wait_torch(a.device)
        self._chk(self.L.uwspr_frontend_batch(self.h, _ptr(a), B, nin, N.DEVICE if dev else N.HOST, _ptr(out)))
        if dev:
            self._wait_self(always=False)
        return out

    def debug_frontend_launch(self, audio, in0, out, m_first, nch=1, plane=None, nout=None, nin=None):
        """diagnostics: ONE launch of the stream form of K0 (uwspr_debug_frontend_launch; what a stream's audio push
        runs) on torch CUDA tensors.  audio: float32 or int16, audio [in0, in0 + nin) -- nin samples, or nin frames of
        nch interleaved channels (nin defaults to all of it); out: float32, receives outputs [m_first, m_first + nout)
        of channel b at pair b * plane (nout defaults to what `out` holds per channel, plane to nout).  The tensors
        must hold what the launch reads and writes: that is checked here, the library sees pointers only."""
        fmt = _launch_tensors("debug_frontend_launch", audio, out)
        nch = int(nch)
        if nin is None:
            nin = audio.numel() // max(nch, 1)
        if nout is None:
            if plane is not None:
                raise ValueError("debug_frontend_launch: plane without nout")
            nout = out.numel() // (2 * max(nch, 1))
        if plane is None:
            plane = nout
        nin, nout, plane = int(nin), int(nout), int(plane)
        if nin * nch > audio.numel() or 2 * ((nch - 1) * plane + nout) > out.numel():
            raise ValueError("debug_frontend_launch: nin %d x nch %d / nout %d, plane %d do not fit the tensors" % (nin, nch, nout, plane))
        self._wait_torch(audio.device)
        self._chk(self.L.uwspr_debug_frontend_launch(self.h, C.c_void_p(audio.data_ptr()), fmt, nin, int(in0), nch,
                                                     C.c_void_p(out.data_ptr()), nout, int(m_first), plane))

    def debug_frontend_carrier_launch(self, audio, in0, out, m_first, carriers, nch=1, plane=None, nout=None, nin=None):
        """diagnostics: ONE launch of the carrier form of K0 (uwspr_debug_frontend_carrier_launch; what a stream's audio
        push runs for any carriers but {1500 Hz} at 10 Hz) on torch CUDA tensors, in the context's "frontend" mode with its
        "frontend_hbw".  audio: float32 or int16, nin frames [in0, in0 + nin) of nch interleaved channels; carriers: Hz;
        out: float32, receives outputs [m_first, m_first + nout) of plane c * len(carriers) + k at pair plane_index *
        plane.  The tensors must hold what the launch reads and writes: that is checked here."""
        fmt = _launch_tensors("debug_frontend_carrier_launch", audio, out)
        car = np.ascontiguousarray(carriers, np.int32).reshape(-1)
        nch, NC = int(nch), int(car.size)
        if nch < 1 or NC < 1:
            raise ValueError("debug_frontend_carrier_launch: nch %d, %d carriers" % (nch, NC))
        npl = nch * NC
        if nin is None:
            nin = audio.numel() // nch
        if nout is None:
            if plane is not None:
                raise ValueError("debug_frontend_carrier_launch: plane without nout")
            nout = out.numel() // (2 * npl)
        if plane is None:
            plane = nout
        nin, nout, plane = int(nin), int(nout), int(plane)
        if nin < 1 or nout < 1 or plane < nout or nin * nch > audio.numel() or 2 * ((npl - 1) * plane + nout) > out.numel():
            raise ValueError("debug_frontend_carrier_launch: nin %d x nch %d / nout %d, plane %d x %d do not fit the tensors"
                             % (nin, nch, nout, plane, npl))
        self._wait_torch(audio.device)
        self._chk(self.L.uwspr_debug_frontend_carrier_launch(self.h, C.c_void_p(audio.data_ptr()), fmt, nin, int(in0), nch, NC,
                                                             C.c_void_p(car.ctypes.data), C.c_void_p(out.data_ptr()), nout,
                                                             int(m_first), plane))

    # -- resampler (K11) ----------------------------------------------------
    def resample(self, audio, rate, nout=None):
        """Audio at `rate` S/s -> 12 kS/s float32 (uwspr_resample_batch): a 1-D [n] or 2-D [n, C] numpy float32 or
        int16 array (zero outside it) -> [nout] or [nout, C]; nout defaults to ceil(n * 12000 / rate), the outputs
        whose audio time lies inside the record.  A contiguous torch CUDA tensor of those shapes and types stays on the
        device (-> a CUDA tensor)."""
        a, fmt, nch = _audio_block(audio, "resample")
        dev = _is_torch(a)
        if nout is None:
            nout = -(-a.shape[0] * AUDIO_RATE // int(rate))
        out = _empty(a, (int(nout),) + tuple(a.shape[1:]), np.float32)
        if dev:
            self._wait_torch(a.device)
        self._chk(self.L.uwspr_resample_batch(self.h, _ptr(a), a.shape[0], nch, fmt, int(rate), N.DEVICE if dev else N.HOST,
                                              _ptr(out), int(nout)))
        if dev:
            self._wait_self(always=False)
        return out

    def debug_resample_launch(self, audio, rate, in0, out, j_first, nch=1, nin=None, nout=None):
        """diagnostics: ONE launch of K11 (uwspr_debug_resample_launch) on torch CUDA tensors.  audio: float32 or int16,
        frames [in0, in0 + nin) of nch interleaved samples (nin defaults to all of it); out: float32, receives outputs
        [j_first, j_first + nout) as [nout, nch] (nout defaults to what it holds).  The input format picks the kernel's
        instantiation.  The tensors must hold what the launch reads and writes: checked here."""
        fmt = _launch_tensors("debug_resample_launch", audio, out)
        nch = int(nch)
        nin = audio.numel() // nch if nin is None else int(nin)
        nout = out.numel() // nch if nout is None else int(nout)
        if nin * nch > audio.numel() or nout * nch > out.numel():
            raise ValueError("debug_resample_launch: nin %d / nout %d x nch %d do not fit the tensors" % (nin, nout, nch))
        self._wait_torch(audio.device)
        self._chk(self.L.uwspr_debug_resample_launch(self.h, C.c_void_p(audio.data_ptr()), fmt, nin, int(in0), nch, int(rate),
                                                     C.c_void_p(out.data_ptr()), nout, int(j_first)))

    # -- blanker (K12) ------------------------------------------------------
    def blank(self, x, blank=24, guard=2):
        """Impulses out of audio at any rate (uwspr_blank_batch): a 1-D [n] or 2-D [n, C] numpy float32 or int16 array
        -> (y float32 of the same shape, med float32 [nblocks] or [nblocks, C]: the level of every complete block of
        4096 samples, nzero int32 of that shape: the outputs of the block set to zero).  A contiguous torch CUDA tensor
        of those shapes and types stays on the device (-> CUDA tensors)."""
        a, fmt, nch = _audio_block(x, "blank")
        dev = _is_torch(a)
        blocks = (-(-a.shape[0] // BLANK_BLOCK),) + tuple(a.shape[1:])
        y, med, nz = _empty(a, a.shape, np.float32), _empty(a, blocks, np.float32), _empty(a, blocks, np.int32)
        if dev:
            self._wait_torch(a.device)
        self._chk(self.L.uwspr_blank_batch(self.h, _ptr(a), a.shape[0], nch, fmt, N.DEVICE if dev else N.HOST, int(blank),
                                           int(guard), _ptr(y), _ptr(med), _ptr(nz)))
        if dev:
            self._wait_self(always=False)
        return y, med, nz

    def stream_blank_stats(self, channels=1):
        """uwspr_stream_blank_stats: per channel, (samples output, samples set to zero) by the stream's blanker since
        open / reset -> two int64 arrays [channels]; zeros when option "blank" is 0"""
        s, z = np.zeros(int(channels), np.int64), np.zeros(int(channels), np.int64)
        rc = self.L.uwspr_stream_blank_stats(self.h, C.c_void_p(s.ctypes.data), C.c_void_p(z.ctypes.data), int(channels))
        if rc < 0:   # (>= 0: the stream's channel count)
            self._chk(rc)
        return s, z

    def debug_blank_launch(self, audio, in0, lev, blk0, level_first, level_n, blank, guard, out, y_first, nz, nch=1, nin=None,
                           nout=None):
        """diagnostics: ONE launch of each K12 kernel (uwspr_debug_blank_launch) on torch CUDA tensors.  audio: float32
        or int16, frames [in0, in0 + nin) of nch interleaved samples (nin defaults to all of it); lev: float32 level
        table [rows, nch] whose row 0 is block blk0; k12_level writes the levels of blocks [level_first, level_first +
        level_n) into it (level_n = 0: no launch), then k12_apply makes outputs [y_first, y_first + nout) into out
        (float32 [nout, nch]; nout defaults to what it holds, 0 or out=None: no launch) and their zero counts into nz
        (int32 [blocks touched, nch]).  The tensors must hold what the launches read and write: checked here."""
        import torch
        fmt = _launch_tensors("debug_blank_launch", audio)
        if lev.dtype != torch.float32 or not lev.is_cuda or not lev.is_contiguous():
            raise TypeError("debug_blank_launch: lev is a contiguous float32 CUDA tensor")
        nch = int(nch)
        nin = audio.numel() // nch if nin is None else int(nin)
        nlev = lev.numel() // nch
        if out is None:
            nout = 0
        else:
            if out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or nz.dtype != torch.int32 or not nz.is_cuda or not nz.is_contiguous():
                raise TypeError("debug_blank_launch: out / nz are contiguous float32 / int32 CUDA tensors")
            nout = out.numel() // nch if nout is None else int(nout)
        nblk = (int(y_first) + nout - 1) // BLANK_BLOCK - int(y_first) // BLANK_BLOCK + 1 if nout > 0 else 0
        if nin * nch > audio.numel() or (nout > 0 and (nout * nch > out.numel() or nblk * nch > nz.numel())):
            raise ValueError("debug_blank_launch: nin %d / nout %d x nch %d do not fit the tensors" % (nin, nout, nch))
        self._wait_torch(audio.device)
        self._chk(self.L.uwspr_debug_blank_launch(self.h, C.c_void_p(audio.data_ptr()), fmt, nin, int(in0), nch,
                                                  C.c_void_p(lev.data_ptr()), nlev, int(blk0), int(level_first), int(level_n),
                                                  int(blank), int(guard), C.c_void_p(out.data_ptr() if nout > 0 else None), nout,
                                                  int(y_first), C.c_void_p(nz.data_ptr() if nout > 0 else None)))

    # -- FDR ---------------------------------------------------------------
    def fdr_batch(self, frames):
        """-> list (per frame) of candidate record arrays, FDR_impl.cc:214-456."""
        p, B, where, keep = self._frames(frames)
        cands, npk = self._cand_buffers(B, frames.device if where == N.DEVICE else None)
        self._chk(self.L.uwspr_fdr_batch(self.h, p, B, where, _ptr(cands), _ptr(npk)))
        if where == N.DEVICE:
            self._wait_self(always=True)
        return _cand_lists(cands, npk)

    def fdr_from_ps(self, ps_band):
        """diagnostics: the spectrum kernel and the coarse search on a GIVEN spectrogram, ps_band [B, n, band_w] float32
        (the layout fdr_spectrum returns; a numpy array or a torch CUDA tensor) -> what fdr_batch returns."""
        i = self.info
        if _is_torch(ps_band):
            import torch
            assert ps_band.is_cuda and ps_band.is_contiguous() and ps_band.dtype == torch.float32
            a, B, where = ps_band, ps_band.numel() // (i.n * i.band_w), N.DEVICE
            assert B * i.n * i.band_w == ps_band.numel()
            self._wait_torch(ps_band.device)
        else:
            a = np.ascontiguousarray(ps_band, dtype=np.float32).reshape(-1, i.n, i.band_w)
            B, where = a.shape[0], N.HOST
        cands, npk = self._cand_buffers(B, a.device if where == N.DEVICE else None)
        self._chk(self.L.uwspr_debug_fdr_from_ps(self.h, _ptr(a), B, where, _ptr(cands), _ptr(npk)))
        if where == N.DEVICE:
            self._wait_self(always=True)
        return _cand_lists(cands, npk)

    def fdr_spectrum(self, B):
        i = self.info
        ps = np.empty((B, i.n, i.band_w), np.float32)
        psavg = np.empty((B, i.band_w), np.float32)
        smraw = np.empty((B, i.finpb), np.float32)
        smspec = np.empty((B, i.finpb), np.float32)
        noise = np.empty(B, np.float32)
        self._chk(self.L.uwspr_fdr_read_spectrum(self.h, B, *[C.c_void_p(a.ctypes.data) for a in
                                                              (ps, psavg, smraw, smspec, noise)]))
        return ps, psavg, smraw, smspec, noise

    def keep_syncgrid(self, ncand_cap):
        self._chk(self.L.uwspr_fdr_keep_syncgrid(self.h, ncand_cap))
        self._grid_cap = ncand_cap

    def fdr_syncgrid(self, B):
        g = np.empty((B, self._grid_cap, N.NIFR, N.NK0, self.info.cell_hyps), np.float32)
        self._chk(self.L.uwspr_fdr_read_syncgrid(self.h, B, C.c_void_p(g.ctypes.data)))
        return g

    # -- fine sweep --------------------------------------------------------
    def sync_sweep(self, frames, hyps, soft=True):
        """hyps: HYP_DTYPE array. -> (sync[H], symbols[H,162] or None)."""
        p, B, where, keep = self._frames(frames)
        hyps = np.ascontiguousarray(hyps, dtype=N.HYP_DTYPE)
        H = hyps.size
        if where == N.DEVICE:
            import torch
            dh = torch.from_numpy(np.frombuffer(hyps.tobytes(), np.uint8).copy()).to(frames.device)
            sync = torch.empty(H, dtype=torch.float32, device=frames.device)
            sym = torch.empty(H * N.NSYM, dtype=torch.uint8, device=frames.device) if soft else None
            self._chk(self.L.uwspr_sync_sweep(self.h, p, B, C.c_void_p(dh.data_ptr()), H, where,
                                              C.c_void_p(sync.data_ptr()),
                                              C.c_void_p(sym.data_ptr()) if soft else None))
            self._wait_self(always=True)
            return sync.cpu().numpy(), (sym.cpu().numpy().reshape(H, N.NSYM) if soft else None)
        sync = np.empty(H, np.float32)
        sym = np.empty((H, N.NSYM), np.uint8) if soft else None
        self._chk(self.L.uwspr_sync_sweep(self.h, p, B, C.c_void_p(hyps.ctypes.data), H, where,
                                          C.c_void_p(sync.ctypes.data),
                                          C.c_void_p(sym.ctypes.data) if soft else None))
        return sync, sym

    def sync_grid(self, frames, centres, df, ddrift, dlag, soft=True, into=None):
        """(freq, drift, lag) grid around one centre per frame (uwspr_sync_grid).
        -> sync [B,nf,ndrift,nlag], symbols [B,nf,ndrift,nlag,162] (numpy), or, with
        device frames and into=(sync_t, sym_t), results left in those torch tensors."""
        p, B, where, keep = self._frames(frames)
        df = np.ascontiguousarray(df, np.float32)
        ddrift = np.ascontiguousarray(ddrift, np.float32)
        dlag = np.ascontiguousarray(dlag, np.int32)
        shape = (B, df.size, ddrift.size, dlag.size)
        H = int(np.prod(shape))
        args = (df.size, C.c_void_p(df.ctypes.data), ddrift.size, C.c_void_p(ddrift.ctypes.data),
                dlag.size, C.c_void_p(dlag.ctypes.data))
        if where == N.DEVICE:
            import torch
            if _is_torch(centres):
                cent_t = centres
            else:
                cent = np.ascontiguousarray(centres, dtype=N.CAND_DTYPE)
                cent_t = torch.from_numpy(np.frombuffer(cent.tobytes(), np.uint8).copy()).to(frames.device)
            if into is None:
                sync_t = torch.empty(H, dtype=torch.float32, device=frames.device)
                sym_t = torch.empty(H * N.NSYM, dtype=torch.uint8, device=frames.device) if soft else None
            else:
                sync_t, sym_t = into
            self._chk(self.L.uwspr_sync_grid(self.h, p, B, where, C.c_void_p(cent_t.data_ptr()), *args,
                                             C.c_void_p(sync_t.data_ptr()),
                                             C.c_void_p(sym_t.data_ptr()) if sym_t is not None else None))
            if into is not None:
                return None
            self._wait_self(always=True)
            return (sync_t.cpu().numpy().reshape(shape),
                    sym_t.cpu().numpy().reshape(shape + (N.NSYM,)) if soft else None)
        cent = np.ascontiguousarray(centres, dtype=N.CAND_DTYPE)
        sync = np.empty(shape, np.float32)
        sym = np.empty(shape + (N.NSYM,), np.uint8) if soft else None
        self._chk(self.L.uwspr_sync_grid(self.h, p, B, where, C.c_void_p(cent.ctypes.data), *args,
                                         C.c_void_p(sync.ctypes.data),
                                         C.c_void_p(sym.ctypes.data) if soft else None))
        return sync, sym

    def sync_and_demodulate(self, frames, calls):
        """calls: CALL_DTYPE array, one per sync_and_demodulate() invocation
        (sync_and_demodulate_impl.cc:126-131). -> RESULT_DTYPE array."""
        p, B, where, keep = self._frames(frames)
        calls = np.ascontiguousarray(calls, dtype=N.CALL_DTYPE)
        res = np.zeros(calls.size, N.RESULT_DTYPE)
        self._chk(self.L.uwspr_sync_and_demodulate_batch(self.h, p, B, where,
                                                         C.c_void_p(calls.ctypes.data), calls.size,
                                                         C.c_void_p(res.ctypes.data)))
        return res

    # -- schedule ----------------------------------------------------------
    def demod_batch(self, frames, cands_per_frame, max_per_frame=1):
        p, B, where, keep = self._frames(frames)
        assert where == N.HOST, "demod_batch with device frames: use pipeline_batch"
        stride = max(1, max(len(c) for c in cands_per_frame))
        cands = np.zeros((B, stride), N.CAND_DTYPE)
        npk = np.zeros(B, np.int32)
        for b, c in enumerate(cands_per_frame):
            cands[b, :len(c)] = c
            npk[b] = len(c)
        out = np.zeros((B, max_per_frame), N.DEMOD_DTYPE)
        self._chk(self.L.uwspr_demod_batch(self.h, p, B, where, C.c_void_p(cands.ctypes.data),
                                           C.c_void_p(npk.ctypes.data), stride, max_per_frame,
                                           C.c_void_p(out.ctypes.data)))
        return out

    # ---- overlap-aware stream ingest (uwspr_stream_*) ----
    def stream_open(self, hop=3375, max_frames=256):
        self._chk(self.L.uwspr_stream_open(self.h, int(hop), int(max_frames)))

    def stream_push(self, iq):
        """Append (I,Q) samples (numpy [n,2] float32, or a torch CUDA tensor); -> frames ready."""
        n = C.c_int(0)
        if _is_torch(iq):
            self._chk(self.L.uwspr_stream_push(self.h, C.c_void_p(iq.data_ptr()), iq.numel() // 2, N.DEVICE, C.byref(n)))
        else:
            a = np.ascontiguousarray(iq, np.float32)
            self._chk(self.L.uwspr_stream_push(self.h, C.c_void_p(a.ctypes.data), a.size // 2, N.HOST, C.byref(n)))
        return n.value

    def stream_push_audio(self, x, where="host"):
        """Append 12 kS/s real audio (uwspr_stream_push_audio): a 1-D numpy float32 or int16 array, or a torch CUDA
        float32 / int16 tensor; -> frames ready.  Stream sample m is the front-end's output at audio index 32 m.
        A page-locked array (host_alloc) goes as one DMA; where="async" only enqueues it (keep it unchanged until
        stream_wait_uploads())."""
        n = C.c_int(0)
        if _is_torch(x):
            fmt = _audio_format(x)
            if fmt is None or x.dim() != 1 or not x.is_cuda:
                raise TypeError("stream_push_audio: a 1-D float32 or int16 CUDA tensor, not %s %s" % (x.dtype, tuple(x.shape)))
            copied = not x.is_contiguous()
            x = x.contiguous()
            self._wait_torch(x.device)
            self._chk(self.L.uwspr_stream_push_audio(self.h, C.c_void_p(x.data_ptr()), x.numel(), fmt, N.DEVICE, C.byref(n)))
            if copied:   # the copy stream reads the temporary after this call returns: keep it until it has
                self.stream_wait_uploads()
            return n.value
        a = _audio_array(x)
        self._chk(self.L.uwspr_stream_push_audio(self.h, C.c_void_p(a.ctypes.data), a.size, _audio_format(a),
                                                 {"host": N.HOST, "async": N.HOST_ASYNC}[where], C.byref(n)))
        return n.value

    def stream_reset(self, pos=0):
        """uwspr_stream_reset: drop what is buffered; the next sample pushed has stream index pos (audio: audio
        index 32 pos, after a zero history)"""
        self._chk(self.L.uwspr_stream_reset(self.h, int(pos)))

    def stream_take(self, nframes, into):
        """The next nframes frames into a torch CUDA float32 tensor [nframes, fl, 2]; -> stream
        index of the first frame's first sample."""
        pos = C.c_longlong(0)
        fr = C.c_void_p()
        self._chk(self.L.uwspr_stream_take(self.h, int(nframes), C.c_void_p(into.data_ptr()), C.byref(fr), C.byref(pos)))
        return pos.value

    def stream_take_view(self, nframes):
        """The next nframes frames IN PLACE -> (device pointer, stride in samples, stream index of
        the first frame).  Frame j starts at pointer + 8*stride*j bytes; valid until the next take.
        Use with set_frame_stride(stride) and frames_ptr=... of the *_into calls."""
        pos = C.c_longlong(0)
        fr = C.c_void_p()
        st = C.c_int(0)
        self._chk(self.L.uwspr_stream_take_view(self.h, int(nframes), C.byref(fr), C.byref(st), C.byref(pos)))
        return fr.value, st.value, pos.value

    def stream_wait_uploads(self):
        self._chk(self.L.uwspr_stream_wait_uploads(self.h))

    def set_frame_stride(self, stride=0):
        """Frame pitch in samples of the `frames` argument of the calls that follow (0 = fl)."""
        self._chk(self.L.uwspr_set_frame_stride(self.h, int(stride)))

    def set_tries(self, ntries):
        """Mode-2 tries per candidate the schedule calls produce (17 = all; fewer = lazy)."""
        self._chk(self.L.uwspr_set_tries(self.h, int(ntries)))

    def demod_resume(self, frames, need, out, max_per_frame=1):
        """Produce all 17 tries for the slots flagged in `need` (uint8 [B, max_per_frame]) of the
        last schedule call.  Host form: returns the full record array; device form (torch
        tensors for need / out): in place."""
        p, B, where, keep = self._frames(frames)
        if where == N.DEVICE:
            self._chk(self.L.uwspr_demod_resume(self.h, p, B, where, C.c_void_p(need.data_ptr()),
                                                max_per_frame, C.c_void_p(out.data_ptr())))
            return out
        need = np.ascontiguousarray(need, np.uint8).reshape(B, max_per_frame)
        res = np.zeros((B, max_per_frame), N.DEMOD_DTYPE)
        self._chk(self.L.uwspr_demod_resume(self.h, p, B, where, C.c_void_p(need.ctypes.data),
                                            max_per_frame, C.c_void_p(res.ctypes.data)))
        return res

    def pipeline_batch(self, frames, max_per_frame=1, fetch=True):
        """FDR + refinement schedule. -> (cands list, demod_out[B,max_per_frame]) or None."""
        p, B, where, keep = self._frames(frames)
        if where == N.DEVICE:
            import torch
            if not fetch:
                self._chk(self.L.uwspr_pipeline_batch(self.h, p, B, where, max_per_frame, None,
                                                      None, None))
                return None
            cands, npk = self._cand_buffers(B, frames.device)
            out = torch.empty(B * max_per_frame * N.DEMOD_DTYPE.itemsize, dtype=torch.uint8, device=frames.device)
        else:
            cands, npk = self._cand_buffers(B)
            out = np.zeros((B, max_per_frame), N.DEMOD_DTYPE)
        self._chk(self.L.uwspr_pipeline_batch(self.h, p, B, where, max_per_frame, _ptr(cands), _ptr(npk), _ptr(out)))
        if where == N.DEVICE:
            self._wait_self(always=True)
            out = np.frombuffer(out.cpu().numpy().tobytes(), N.DEMOD_DTYPE).reshape(B, -1)
        return _cand_lists(cands, npk), out.copy()

    def pipeline_batch_into(self, frames, cands_t, npk_t, out_t, max_per_frame=1):
        """Device-resident form used by bench.py: frames and the three output
        buffers are torch CUDA tensors; nothing is copied to the host and the call
        returns as soon as the work is enqueued on the context's stream."""
        p, B, where, keep = self._frames(frames)
        assert where == N.DEVICE
        assert cands_t.numel() * cands_t.element_size() >= B * self.maxfreqs * 48
        assert out_t.numel() * out_t.element_size() >= B * max_per_frame * N.DEMOD_DTYPE.itemsize
        self._chk(self.L.uwspr_pipeline_batch(self.h, p, B, where, max_per_frame,
                                              C.c_void_p(cands_t.data_ptr()),
                                              C.c_void_p(npk_t.data_ptr()),
                                              C.c_void_p(out_t.data_ptr())))

    def pipeline_slabs(self, K, slab_t):
        """The next pipeline_batch* call also writes its frames' gather slabs into slab_t (torch CUDA uint8
        [B, 32+48K]); None cancels."""
        self._chk(self.L.uwspr_pipeline_slabs(self.h, int(K), C.c_void_p(slab_t.data_ptr()) if slab_t is not None else None))

    def pack_slabs_into(self, B, K, slab_t):
        """Per-frame gather slabs of the last pipeline batch, written into a torch
        CUDA uint8 tensor [B, 32+48K] (or a numpy array for the host form)."""
        if _is_torch(slab_t):
            self._chk(self.L.uwspr_pack_slabs(self.h, B, K, C.c_void_p(slab_t.data_ptr()), N.DEVICE))
        else:
            self._chk(self.L.uwspr_pack_slabs(self.h, B, K, C.c_void_p(slab_t.ctypes.data), N.HOST))

    def sync_sweep_into(self, frames, hyps_t, H, sync_t, sym_t):
        p, B, where, keep = self._frames(frames)
        assert where == N.DEVICE
        self._chk(self.L.uwspr_sync_sweep(self.h, p, B, C.c_void_p(hyps_t.data_ptr()), H, where,
                                          C.c_void_p(sync_t.data_ptr()),
                                          C.c_void_p(sym_t.data_ptr()) if sym_t is not None else None))

    # -- known-symbol subtraction (K8: uwspr_subtract_batch) -----------------
    def subtract(self, frames, items, refine=True, out=None):
        """Take decoded transmissions out of their frames.  items: a SUB_ITEM_DTYPE array, or dicts with "frame", "shift",
        "f" (Hz), "drift" (Hz, 0) and "symbols" (162 values 0..3) or "text" / "message"; sorted by frame, the items of one
        frame applied in list order.  -> (frames_out, results): numpy [B, fl, 2] for host frames, a torch CUDA tensor for
        device frames (`out`: the tensor to write, which may be `frames` itself), and a SUB_RESULT_DTYPE array."""
        it = sub_items(items)
        p, B, where, keep = self._frames(frames)
        res = np.zeros(len(it), N.SUB_RESULT_DTYPE)
        ip = C.c_void_p(it.ctypes.data) if len(it) else None
        rp = C.c_void_p(res.ctypes.data) if len(it) else None
        if where == N.DEVICE:
            import torch
            if _is_torch(frames):
                if out is None:
                    out = torch.empty((B, self.fl, 2), dtype=torch.float32, device=frames.device)
                assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= 2 * B * self.fl
                op = C.c_void_p(out.data_ptr())
            else:
                assert out is not None, "subtract: a FrameView of device memory needs out"
                op = C.c_void_p(out.data_ptr() if _is_torch(out) else int(out))
            # (results to the host, the frames stay where they are)
            self._chk(self.L.uwspr_subtract_batch(self.h, p, B, N.DEVICE_FRAMES, ip, len(it), 1 if refine else 0, op, rp))
            return out, res
        if out is None:
            out = np.empty((B, self.fl, 2), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.size >= 2 * B * self.fl
        self._chk(self.L.uwspr_subtract_batch(self.h, p, B, N.HOST, ip, len(it), 1 if refine else 0,
                                              C.c_void_p(out.ctypes.data), rp))
        return out, res

    # -- the scored fallbacks: K9, K13, K14 on soft-symbol vectors -------------
    def _scored(self, fn, R, symbols, *extra):
        """fn(ctx, symbols, n, where, *extra, results) on [n, 162] uint8 soft-symbol vectors, a numpy array or a torch CUDA
        tensor (read in place) -> the n results, a numpy array of dtype R"""
        if _is_torch(symbols):
            import torch
            assert symbols.is_cuda and symbols.is_contiguous() and symbols.dtype == torch.uint8
            n = symbols.numel() // N.NSYM
            out = torch.zeros(max(n, 1) * R.itemsize, dtype=torch.uint8, device=symbols.device)
            self._wait_torch(symbols.device)
            self._chk(fn(self.h, C.c_void_p(symbols.data_ptr()), n, N.DEVICE, *extra, C.c_void_p(out.data_ptr())))
            self._wait_self(always=True)
            return out.cpu().numpy()[:n * R.itemsize].view(R).copy()
        a = np.ascontiguousarray(symbols, dtype=np.uint8).reshape(-1, N.NSYM)
        res = np.zeros(len(a), R)
        self._chk(fn(self.h, C.c_void_p(a.ctypes.data) if len(a) else None, len(a), N.HOST, *extra,
                     C.c_void_p(res.ctypes.data) if len(a) else None))
        return res

    # -- ordered-statistics decoding (K9: uwspr_osd_batch) -------------------
    def osd(self, symbols, order=2):
        """Ordered-statistics decoding of soft-symbol vectors as uwspr_demod_out.symbols[idt] holds them: [n, 162] uint8, a
        numpy array or a torch CUDA tensor (read in place).  -> an OSD_RESULT_DTYPE array: dmin, dnext, nhard, nflip and
        the 7 message bytes per vector (include/uwspr_hip.h states the definition)."""
        return self._scored(self.L.uwspr_osd_batch, N.OSD_RESULT_DTYPE, symbols, int(order))

    # -- list search (K13: uwspr_deep_set_list, uwspr_deep_batch) -------------
    def deep_set_list(self, known):
        """The list of expected messages: WSPR texts (packed with wspr_pack) or an [M, 7] int8 array of packed messages;
        empty clears it.  Distinct 50-bit messages, at most native.DEEP_MAX (include/uwspr_hip.h states the rules)."""
        m = deep_list(known)
        self._chk(self.L.uwspr_deep_set_list(self.h, C.c_void_p(m.ctypes.data) if len(m) else None, len(m)))

    def deep(self, symbols):
        """Soft-symbol vectors as uwspr_demod_out.symbols[idt] holds them -- [n, 162] uint8, a numpy array or a torch CUDA
        tensor (read in place) -- scored against every codeword of the list.  -> a DEEP_RESULT_DTYPE array: best (index
        in the list), sbest, snext per vector (include/uwspr_hip.h states the definition)."""
        return self._scored(self.L.uwspr_deep_batch, N.DEEP_RESULT_DTYPE, symbols)

    # -- call search (K14: uwspr_calls_set, uwspr_calls_batch) -----------------
    def calls_set(self, calls, grids=None, powers=None):
        """The call set: callsigns of type-1 messages (1 to native.CALLS_MAX, distinct; empty clears it), any locator and
        power unless restricted: grids = 2-character fields ("FN") and / or 4-character locators ("FN42"), powers = a subset
        of native.P19 in dBm (include/uwspr_hip.h states the rules)."""
        arr, A, bm, pm = calls_args(calls, grids, powers)
        self._chk(self.L.uwspr_calls_set(self.h, arr, A, C.c_void_p(bm.ctypes.data) if bm is not None else None, pm))

    def calls(self, symbols):
        """Soft-symbol vectors as at Context.deep -- [n, 162] uint8, a numpy array or a torch CUDA tensor (read in place) --
        scored against every allowed (callsign, locator, power) of the call set.  -> a CALL_RESULT_DTYPE array: best (the
        hypothesis index h), call (index), ngrid, dbm, sbest, snext per vector (include/uwspr_hip.h states the definition)."""
        return self._scored(self.L.uwspr_calls_batch, N.CALL_RESULT_DTYPE, symbols)

    # -- block demodulation (K10: uwspr_blockdemod_batch) ---------------------
    def blockdemod(self, frames, items):
        """Soft symbols coherent over 1, 2 and 3 symbols.  items: a BLOCK_ITEM_DTYPE array, or dicts with "frame", "shift",
        "f" (Hz) and "drift" (Hz, 0), sorted by frame; frames: numpy, a torch CUDA tensor or a FrameView.  -> numpy
        [n, 3, 162] uint8: per item the vectors of block length 1, 2, 3, each as uwspr_demod_out.symbols[idt] holds one
        (include/uwspr_hip.h states the definition)."""
        it = block_items(items)
        p, B, where, keep = self._frames(frames)
        ip = C.c_void_p(it.ctypes.data) if len(it) else None
        if where == N.DEVICE:   # device frames: the bytes are written to device memory and copied back
            import torch
            dev = torch.zeros(max(3 * N.NSYM * len(it), 1), dtype=torch.uint8, device=frames.device)
            self._wait_torch(dev.device, always=True)
            self._chk(self.L.uwspr_blockdemod_batch(self.h, p, B, N.DEVICE_FRAMES, ip, len(it), C.c_void_p(dev.data_ptr())))
            return dev.cpu().numpy()[:3 * N.NSYM * len(it)].reshape(len(it), 3, N.NSYM).copy()
        out = np.zeros((len(it), 3, N.NSYM), np.uint8)
        self._chk(self.L.uwspr_blockdemod_batch(self.h, p, B, N.HOST, ip, len(it), C.c_void_p(out.ctypes.data) if len(it) else None))
        return out

    # -- trajectory fit of a decoded source (K15: uwspr_track_set, uwspr_track_batch) ----
    def track_set(self, trajs, qf=4, model="delay"):
        """The trajectory set: (v, d, tc) entries (track_trajs: tuples, dicts, an [n, 3] array or track_grid's result), 1 to
        native.TRACK_MAX of them; qf: frequency offsets -qf .. qf of 0.0125 Hz around each; model "delay" (Doppler and time
        compression) or "doppler" (include/uwspr_hip.h states the rules)."""
        tr = track_trajs(trajs)
        self._chk(self.L.uwspr_track_set(self.h, C.c_void_p(tr.ctypes.data) if len(tr) else None, len(tr), int(qf), _track_model(model)))
        self._track = (len(tr), 2 * int(qf) + 1)

    def track(self, frames, items, surface=False):
        """Fit the set's trajectories to decoded transmissions.  items: Context.subtract's (a SUB_ITEM_DTYPE array, or dicts
        with "frame", "shift", "f", "drift" and "symbols" / "text" / "message"), sorted by frame; frames: numpy, a torch CUDA
        tensor or a FrameView.  -> a TRACK_RESULT_DTYPE array (best = trajectory * nf + offset index, t_best, t_ref, f_hz),
        and with surface=True also T of every hypothesis, numpy [nitems, n, nf] float32."""
        it = sub_items(items)
        n, nf = getattr(self, "_track", (0, 1))
        p, B, where, keep = self._frames(frames)
        ip = C.c_void_p(it.ctypes.data) if len(it) else None
        if where == N.DEVICE:   # device frames: the results are written to device memory and copied back
            import torch
            dev = frames.device
            res = torch.zeros(max(len(it), 1) * N.TRACK_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            surf = torch.zeros(max(len(it) * n * nf, 1), dtype=torch.float32, device=dev) if surface else None
            self._wait_torch(dev, always=True)
            self._chk(self.L.uwspr_track_batch(self.h, p, B, N.DEVICE_FRAMES, ip, len(it), C.c_void_p(res.data_ptr()),
                                               C.c_void_p(surf.data_ptr()) if surface else None))
            out = res.cpu().numpy()[:len(it) * N.TRACK_RESULT_DTYPE.itemsize].view(N.TRACK_RESULT_DTYPE).copy()
            return (out, surf.cpu().numpy()[:len(it) * n * nf].reshape(len(it), n, nf).copy()) if surface else out
        out = np.zeros(len(it), N.TRACK_RESULT_DTYPE)
        surf = np.zeros((len(it), n, nf), np.float32) if surface else None
        self._chk(self.L.uwspr_track_batch(self.h, p, B, N.HOST, ip, len(it), C.c_void_p(out.ctypes.data) if len(it) else None,
                                           C.c_void_p(surf.ctypes.data) if surface and surf.size else None))
        return (out, surf) if surface else out

    # -- blind demodulation along straight-line passes (K16: uwspr_follow_set, uwspr_follow_batch) ----
    def follow_set(self, grid, qf=8, lags=1, model="doppler"):
        """The follow set: (v, d, tc) passes as at track_set; qf: frequency offsets -qf .. qf of 375/2048 Hz (0 .. 16);
        lags: -lags .. lags steps of 32 samples (0 .. 4); model "doppler" or "delay" (include/uwspr_hip.h states the rules)."""
        tr = track_trajs(grid)
        self._chk(self.L.uwspr_follow_set(self.h, C.c_void_p(tr.ctypes.data) if len(tr) else None, len(tr), int(qf), int(lags), _track_model(model)))
        self._follow = (len(tr), 2 * int(qf) + 1, 2 * int(lags) + 1)

    def follow(self, frames, items, surface=False):
        """Demodulate records blind along the set's passes.  items: Context.blockdemod's (a BLOCK_ITEM_DTYPE array, or dicts
        with "frame", "shift", "f", "drift"), sorted by frame; frames: numpy, a torch CUDA tensor or a FrameView.  -> (a
        FOLLOW_RESULT_DTYPE array (best = (trajectory * nf + offset index) * nlg + lag index, s_best, s_ref, f_hz), the soft
        symbols of the best hypothesis, numpy [nitems, 162] uint8 as uwspr_demod_out.symbols[idt] holds a vector), and with
        surface=True also S of every hypothesis, numpy [nitems, n, nf, nlg] float32."""
        it = block_items(items)
        n, nf, nlg = getattr(self, "_follow", (0, 1, 1))
        p, B, where, keep = self._frames(frames)
        ip = C.c_void_p(it.ctypes.data) if len(it) else None
        nh = n * nf * nlg
        if where == N.DEVICE:   # device frames: the results are written to device memory and copied back
            import torch
            dev = frames.device
            res = torch.zeros(max(len(it), 1) * N.FOLLOW_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            sym = torch.zeros(max(len(it), 1) * N.NSYM, dtype=torch.uint8, device=dev)
            surf = torch.zeros(max(len(it) * nh, 1), dtype=torch.float32, device=dev) if surface else None
            self._wait_torch(dev, always=True)
            self._chk(self.L.uwspr_follow_batch(self.h, p, B, N.DEVICE_FRAMES, ip, len(it), C.c_void_p(res.data_ptr()),
                                                C.c_void_p(sym.data_ptr()), C.c_void_p(surf.data_ptr()) if surface else None))
            out = res.cpu().numpy()[:len(it) * N.FOLLOW_RESULT_DTYPE.itemsize].view(N.FOLLOW_RESULT_DTYPE).copy()
            osym = sym.cpu().numpy()[:len(it) * N.NSYM].reshape(len(it), N.NSYM).copy()
            return (out, osym, surf.cpu().numpy()[:len(it) * nh].reshape(len(it), n, nf, nlg).copy()) if surface else (out, osym)
        out = np.zeros(len(it), N.FOLLOW_RESULT_DTYPE)
        osym = np.zeros((len(it), N.NSYM), np.uint8)
        surf = np.zeros((len(it), n, nf, nlg), np.float32) if surface else None
        self._chk(self.L.uwspr_follow_batch(self.h, p, B, N.HOST, ip, len(it), C.c_void_p(out.ctypes.data) if len(it) else None,
                                            C.c_void_p(osym.ctypes.data) if len(it) else None,
                                            C.c_void_p(surf.ctypes.data) if surface and surf.size else None))
        return (out, osym, surf) if surface else (out, osym)

    # -- transmit side (K7: uwspr_tx_*) ------------------------------------
    def tx_baseband(self, signals, n=45000, t0=0, channel=0, out=None):
        """375 S/s baseband samples [t0, t0 + n) of one channel's signals (tx_signals), as c2_read returns a .c2 file:
        numpy [n, 2] float32, or written into `out` (a torch CUDA float32 tensor of n pairs).  A signal with a "motion"
        (tx_motions) sends the call through uwspr_tx_baseband_moving, one with a "carrier" (tx_carriers: Hz; here it
        only scales a motion's Doppler, the baseband is not rotated) through uwspr_tx_baseband_at, one with a "fading"
        (tx_fades) through uwspr_tx_baseband_medium."""
        signals = list(signals)
        sig, mot, car, fad = tx_signals(signals), tx_motions(signals), tx_carriers(signals), tx_fades(signals)
        route = (self.L, "baseband", self.h, sig, mot, car, fad, None)
        if out is not None and _is_torch(out):
            import torch
            if not (out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= 2 * n):
                raise TypeError("tx_baseband: out must be a contiguous float32 CUDA tensor of >= %d elements, not %s %s"
                                % (2 * n, out.dtype, tuple(out.shape)))
            self._wait_torch(out.device)
            self._chk(_tx_call(*route, len(sig), int(channel), int(t0), int(n), C.c_void_p(out.data_ptr()), N.DEVICE))
            self._wait_self(always=False)
            return out
        iq = np.empty((n, 2), np.float32)
        self._chk(_tx_call(*route, len(sig), int(channel), int(t0), int(n), C.c_void_p(iq.ctypes.data), N.HOST))
        return iq

    def tx_render(self, signals, nframes, t0=0, channels=1, sigma=0.0, seed=0, background=None, background_gain=1.0,
                  format="f32", out=None, impulses=None):
        """12 kS/s audio frames [t0, t0 + nframes) of a `channels`-channel recording (uwspr_tx_render) -> numpy
        [nframes, channels] float32 / int16 (format "f32" / "s16"), or written into `out`, a torch CUDA tensor of that
        shape and dtype (what stream_push_audio / a pipe takes, with no PCIe crossing).  sigma, seed, background
        (a 1-D float32 / int16 numpy array or torch tensor, or None) and background_gain are one value for every channel
        or a list of one per channel.  A background is moved to where the output is made: to out's device for device
        output (once per call: keep it there for repeated renders), to host memory for host output.  A signal with a
        "motion" (tx_motions) sends the call through uwspr_tx_render_moving; one with a "carrier" (tx_carriers: integer
        Hz, 170 .. the option "tx_cutoff" - 250; the others stay at 1500) through uwspr_tx_render_at: the transmission is
        centred on carrier + f0 Hz, and a channel may carry several carriers at once.  A signal with a "fading"
        (tx_fades), or impulses -- a dict {"rate": events per sample, "sigma", "seed": 0, "length": 1} or a list of one
        (or None) per channel: Bernoulli-Gaussian bursts between the AWGN and the background -- send the call through
        uwspr_tx_render_medium."""
        signals = list(signals)
        sig, mot, car, fad = tx_signals(signals), tx_motions(signals), tx_carriers(signals), tx_fades(signals)
        imp = tx_impulses(impulses, int(channels))
        route = (self.L, "render", self.h, sig, mot, car, fad, imp)
        dev_out = out is not None and _is_torch(out)
        if dev_out and not out.is_cuda:
            raise TypeError("tx_render: out must be a CUDA tensor (or None for a numpy result)")
        Cn = int(channels)
        per = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * Cn   # noqa: E731
        sg, sd, bg, bgg = per(sigma), per(seed), per(background), per(background_gain)
        ch = (N.TxChannel * max(Cn, 1))()
        keep, moved = [], False
        for k in range(min(Cn, len(ch))):
            ch[k].sigma, ch[k].seed, ch[k].background_gain = float(sg[k]), int(sd[k]) & (2 ** 64 - 1), float(bgg[k])
            b = bg[k]
            if b is None:
                continue
            if dev_out:
                import torch
                b = b if _is_torch(b) else torch.from_numpy(_audio_array(b))
                if b.dtype not in (torch.float32, torch.int16) or b.dim() != 1:
                    raise TypeError("background: a 1-D float32 or int16 array, not %s %s" % (b.dtype, tuple(b.shape)))
                moved = moved or not b.is_cuda or b.device != out.device or not b.is_contiguous()
                b = b.to(out.device).contiguous()
                ch[k].background, ch[k].background_len = b.data_ptr(), b.numel()
            else:
                if _is_torch(b):
                    b = b.detach().cpu().numpy()
                b = _audio_array(b)
                ch[k].background, ch[k].background_len = b.ctypes.data, b.size
            ch[k].background_format = _audio_format(b)
            keep.append(b)
        fmt = {"f32": N.AUDIO_F32, "s16": N.AUDIO_S16}[format]
        if dev_out:
            import torch
            if not (out.is_contiguous() and out.numel() >= int(nframes) * Cn and
                    out.dtype == (torch.int16 if fmt == N.AUDIO_S16 else torch.float32)):
                raise TypeError("tx_render: out must be a contiguous %s CUDA tensor of >= %d elements, not %s %s"
                                % ("int16" if fmt == N.AUDIO_S16 else "float32", int(nframes) * Cn, out.dtype, tuple(out.shape)))
            self._wait_torch(out.device, always=moved)   # (a moved background was copied on torch's stream)
            self._chk(_tx_call(*route, len(sig), C.byref(ch), Cn, int(t0), int(nframes), fmt, C.c_void_p(out.data_ptr()), N.DEVICE))
            self._wait_self(always=moved)                # (the moved copies are freed when this call returns)
            return out
        a = np.empty((int(nframes), Cn), np.int16 if fmt == N.AUDIO_S16 else np.float32)
        self._chk(_tx_call(*route, len(sig), C.byref(ch), Cn, int(t0), int(nframes), fmt, C.c_void_p(a.ctypes.data), N.HOST))
        return a

    # -- multi-GPU gather over RCCL (uwspr_dist_*) ---------------------------
    @staticmethod
    def dist_unique_id():
        """rank 0: the 128 bytes every rank passes to dist_init (ncclGetUniqueId)."""
        buf = (C.c_char * 128)()
        rc = N.lib().uwspr_dist_unique_id(buf)
        if rc != 0:
            raise N.UwsprError(rc, "uwspr_dist_unique_id: RCCL unavailable")
        return bytes(buf)

    def dist_init(self, rank, world, uid=None):
        self._chk(self.L.uwspr_dist_init(self.h, int(rank), int(world), uid))

    def dist_gather(self, send_t, recv_t=None, root=0):
        """send_t: torch CUDA tensor (this rank's slabs); recv_t: [world * send bytes] on the root."""
        nbytes = send_t.numel() * send_t.element_size()
        self._chk(self.L.uwspr_dist_gather(self.h, C.c_void_p(send_t.data_ptr()), nbytes,
                                           C.c_void_p(recv_t.data_ptr()) if recv_t is not None else None,
                                           int(root), N.DEVICE))

    def dist_finalize(self):
        self._chk(self.L.uwspr_dist_finalize(self.h))

    # -- measurement -------------------------------------------------------
    def prof_enable(self, which=True):
        """which: True = every kernel family, False/0 = off, or an iterable of
        family names from native.K_NAMES (e.g. ("tonecorr",))."""
        if which is True:
            mask = 0x3F
        elif not which:
            mask = 0
        else:
            mask = sum(1 << N.K_NAMES.index(k) for k in which)
        self._chk(self.L.uwspr_prof_enable(self.h, mask))

    def prof_intervals(self, kind, epoch_event_ptr, cap=4096):
        """(start_ms, stop_ms) arrays of the recorded launches of one family, relative
        to a caller-recorded hipEvent (e.g. torch.cuda.Event(enable_timing=True).cuda_event)."""
        a = np.zeros(cap, np.float64)
        b = np.zeros(cap, np.float64)
        n = C.c_int(0)
        self._chk(self.L.uwspr_prof_intervals(self.h, N.K_NAMES.index(kind), C.c_void_p(epoch_event_ptr),
                                              C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data),
                                              cap, C.byref(n)))
        return a[:n.value].copy(), b[:n.value].copy()

    def prof_read(self):
        p = N.Prof()
        self._chk(self.L.uwspr_prof_read(self.h, C.byref(p)))
        return {k: {"ms": p.ms[i], "launches": p.launches[i], "units": p.units[i]}
                for i, k in enumerate(N.K_NAMES)}


# ---- host tail (no device needed) -------------------------------------------
def deinterleave(symbols):
    s = np.array(symbols, dtype=np.uint8).copy()
    N.lib().uwspr_deinterleave(C.c_void_p(s.ctypes.data))
    return s


def fano_decode(symbols, delta=60, maxcycles=10000):
    s = np.ascontiguousarray(symbols, dtype=np.uint8)
    data = np.zeros(11, np.uint8)
    metric, cycles, maxnp = C.c_uint32(), C.c_uint32(), C.c_uint32()
    rc = N.lib().uwspr_fano_decode(C.c_void_p(s.ctypes.data), C.c_void_p(data.ctypes.data),
                                   C.byref(metric), C.byref(cycles), C.byref(maxnp), delta,
                                   maxcycles)
    return rc, data, metric.value, cycles.value


def fano_encode(data_bytes):
    d = np.ascontiguousarray(data_bytes, dtype=np.uint8)
    out = np.zeros(d.size * 16, np.uint8)
    N.lib().uwspr_fano_encode(C.c_void_p(out.ctypes.data), C.c_void_p(d.ctypes.data), d.size)
    return out


def decode_candidate(demod_rec):
    """demod_rec: one DEMOD_DTYPE record. -> (message7 int8 array, idt) or None."""
    rec = np.ascontiguousarray(np.array(demod_rec, dtype=N.DEMOD_DTYPE).reshape(1))
    msg = np.zeros(7, np.int8)
    idt = C.c_int32(-1)
    ok = N.lib().uwspr_decode_candidate(C.c_void_p(rec.ctypes.data), C.c_void_p(msg.ctypes.data),
                                        C.byref(idt))
    return (msg, idt.value) if ok else None


def host_threads():
    """CPUs this process may keep busy (affinity and cgroup quota applied)."""
    return int(N.lib().uwspr_host_threads())


def host_set_ranks(ranks):
    """The `ranks` processes of a job that share this host (LOCAL_WORLD_SIZE) share its CPUs: host_threads() and the
    process-wide Fano pool become that share.  Before the first decode_batch / Pipe of the process."""
    rc = N.lib().uwspr_host_set_ranks(int(ranks))
    if rc != 0:
        raise N.UwsprError(rc, "uwspr_host_set_ranks(%d): %s" % (ranks, "the host pool already exists" if rc == -3 else "ranks < 1"))


def decode_batch(demod_recs, nthreads=0):
    """demod_recs: DEMOD_DTYPE array (any shape). -> (messages [n,7] int8, idt [n] int32,
    decoded [n] bool), record order kept; Fano runs on `nthreads` host threads."""
    rec = np.ascontiguousarray(np.asarray(demod_recs, dtype=N.DEMOD_DTYPE).reshape(-1))
    n = rec.size
    msg = np.zeros((n, 7), np.int8)
    idt = np.full(n, -1, np.int32)
    ok = np.zeros(n, np.uint8)
    rc = N.lib().uwspr_decode_batch(C.c_void_p(rec.ctypes.data), n, nthreads, C.c_void_p(msg.ctypes.data),
                                    C.c_void_p(idt.ctypes.data), C.c_void_p(ok.ctypes.data))
    if rc < 0:
        raise N.UwsprError(rc, "uwspr_decode_batch")
    return msg, idt, ok.astype(bool)


def unpack_message(message7):
    m = np.ascontiguousarray(message7, dtype=np.int8)
    buf = C.create_string_buffer(32)
    rc = N.lib().uwspr_unpack_message(C.c_void_p(m.ctypes.data), buf, 32)
    return rc, buf.value.decode("ascii", "replace")


def host_alloc(nbytes):
    """uwspr_host_alloc: page-locked host memory as a writable ctypes byte array (np.frombuffer it); release with
    host_free."""
    ptr = C.c_void_p()
    rc = N.lib().uwspr_host_alloc(C.c_size_t(nbytes), C.byref(ptr))
    if rc:
        raise N.UwsprError(rc, "uwspr_host_alloc(%d)" % nbytes)
    buf = (C.c_uint8 * nbytes).from_address(ptr.value)
    buf._uwspr_ptr = ptr.value
    return buf


def host_free(buf):
    N.lib().uwspr_host_free(C.c_void_p(buf._uwspr_ptr))


def frontend_design(mode=FRONTEND_GRC, stage=0, centre=1500, half_bw=10):
    """uwspr_frontend_design_at: stage 0 -> (complex128 composite taps g, read-ahead D) of the K0 front-end
    y[m] = sum_k g[k] x[32 m + D - k]; stages 1..3 (grc mode) -> the band-pass, low-pass and resampler designs.
    centre, half_bw: the flowgraph's Center_Frequency and Half_Bandwidth in integer Hz (options "carrier" and
    "frontend_hbw"); away from a multiple of 375 Hz the rotator (frontend_rotator) follows the sum."""
    d = C.c_int32(0)
    centre, half_bw = int(centre), int(half_bw)
    n = N.lib().uwspr_frontend_design_at(mode, centre, half_bw, stage, None, 0, C.byref(d))
    if n < 0:
        raise N.UwsprError(n, "uwspr_frontend_design_at(mode=%d, centre=%d, half_bw=%d, stage=%d)" % (mode, centre, half_bw, stage))
    g = np.zeros(n * (2 if stage == 0 else 1), np.float64)
    N.lib().uwspr_frontend_design_at(mode, centre, half_bw, stage, C.c_void_p(g.ctypes.data), n, C.byref(d))
    if stage == 0:
        return g[0::2] + 1j * g[1::2], int(d.value)
    return g


def tx_taps():
    """diagnostics: K7's filter (uwspr_debug_tx_taps; host only, no device) -> (g complex128 [3179], the composite of
    c2ToWaveFile.grc's chain designed in binary64; image float32 [32, 104, 2], the (Re g, -Im g) tap image the render
    kernel reads: image[p, i] is tap p + 32 i, +0 behind the last one)"""
    g = np.zeros((3179, 2), np.float64)
    image = np.full((32, 104, 2), np.nan, np.float32)
    n = N.lib().uwspr_debug_tx_taps(C.c_void_p(g.ctypes.data), C.c_void_p(image.ctypes.data))
    if n != 3179:
        raise N.UwsprError(n if n < 0 else -1, "uwspr_debug_tx_taps: %d taps, this binding holds 3179" % n)
    return g[:, 0] + 1j * g[:, 1], image


def tx_design(carrier=1500, cutoff=2500):
    """uwspr_tx_design_at (host only, no device): K7's filter at `carrier` Hz with the second low-pass cut off at `cutoff`
    Hz -> (g complex128 [3179], image float32 [32, 104, 2]) as tx_taps returns them; (1500, 2500) is tx_taps' bytes.
    ValueError outside 170 <= carrier <= cutoff - 250, 500 <= cutoff <= 5900."""
    g = np.zeros((3179, 2), np.float64)
    image = np.full((32, 104, 2), np.nan, np.float32)
    n = N.lib().uwspr_tx_design_at(int(carrier), int(cutoff), C.c_void_p(g.ctypes.data), C.c_void_p(image.ctypes.data))
    if n == -6:   # UWSPR_ERR_ARG
        raise ValueError("tx_design: carrier %d Hz with cut-off %d Hz (170 <= carrier <= cutoff - 250, 500 <= cutoff <= 5900)"
                         % (int(carrier), int(cutoff)))
    if n != 3179:
        raise N.UwsprError(n if n < 0 else -1, "uwspr_tx_design_at: %d taps, this binding holds 3179" % n)
    return g[:, 0] + 1j * g[:, 1], image


def _launch_counts(name, n):
    """the n process-wide launch counters uwspr_debug_<name>_counts reads -> a tuple of ints"""
    out = np.zeros(n, np.int64)
    getattr(N.lib(), "uwspr_debug_%s_counts" % name)(C.c_void_p(out.ctypes.data))
    return tuple(int(v) for v in out)


def tx_carrier_launch_counts():
    """diagnostics: launches of K7's carrier form since the process started -> (float32 output, int16 output)"""
    return _launch_counts("tx_carrier", 2)


def tx_medium_launch_counts():
    """diagnostics: launches of K7's medium form since the process started -> (float32 output, int16 output, baseband)"""
    return _launch_counts("tx_medium", 3)


def tx_fade_design(fade):
    """uwspr_tx_fade_design (host only, no device): a "fading" dict (tx_fades) -> (a0, a1, omega float64 [M] in rad per
    baseband sample, phi float64 [M]): the gain is h(k) = a0 + a1 sum_m exp(j (omega_m k + phi_m)), k counted from the
    transmission's first sample.  ValueError outside the ranges include/uwspr_hip.h gives."""
    arr = tx_fades([{"fading": fade}])
    a = np.zeros(2, np.float64)
    om = np.zeros(N.TX_FADE_MAX_PATHS, np.float64)
    ph = np.zeros(N.TX_FADE_MAX_PATHS, np.float64)
    m = N.lib().uwspr_tx_fade_design(C.c_void_p(C.addressof(arr)), C.c_void_p(a.ctypes.data), C.c_void_p(om.ctypes.data),
                                     C.c_void_p(ph.ctypes.data))
    if m < 1:
        raise ValueError("tx_fade_design: %r (spread 0 .. 20 Hz, |shift| <= 20 Hz, k 0 .. 1e6, paths 1 .. 32)" % (fade,))
    return float(a[0]), float(a[1]), om[:m].copy(), ph[:m].copy()


def frontend_rotator():
    """uwspr_frontend_rotator: K0's rotator table -> float32 [375, 2], row i = (cos, -sin)(2 pi i / 375); output m of a
    stream at carrier fc is multiplied by row ((fc mod 375) (m mod 375)) mod 375 unless 375 divides fc"""
    out = np.zeros((375, 2), np.float32)
    n = N.lib().uwspr_frontend_rotator(C.c_void_p(out.ctypes.data))
    if n != 375:
        raise N.UwsprError(n if n < 0 else -1, "uwspr_frontend_rotator")
    return out


def frontend_carrier_launch_counts():
    """diagnostics: launches of K0's carrier form since the process started -> (with float32 input, with int16 input)"""
    return _launch_counts("frontend_carrier", 2)


def resample_design(rate):
    """uwspr_resample_design: the prototype low-pass of the resampler for `rate` S/s -> (taps float64 [N], L, M, T, D);
    ValueError for an unsupported rate."""
    L = N.lib()
    v = [C.c_int(0) for _ in range(4)]
    n = L.uwspr_resample_design(int(rate), None, 0, *[C.byref(q) for q in v])
    if n < 0:
        raise ValueError("audio rate %d S/s is not supported (8000 .. 192000 S/s with 12000 / gcd(rate, 12000) <= 160)" % int(rate))
    taps = np.zeros(n, np.float64)
    L.uwspr_resample_design(int(rate), C.c_void_p(taps.ctypes.data), n, *[C.byref(q) for q in v])
    return (taps,) + tuple(q.value for q in v)


def resample_launch_counts():
    """diagnostics: launches of K11 since the process started -> (with float32 input, with int16 input)"""
    return _launch_counts("resample", 2)


def blank_launch_counts():
    """diagnostics: launches of K12 since the process started -> (k12_level with float32 input, with int16 input,
    k12_apply with float32 input, with int16 input)"""
    return _launch_counts("blank", 4)


def c2_read(path):
    iq = np.zeros((45000, 2), np.float32)
    freq, typ = C.c_double(), C.c_int32()
    rc = N.lib().uwspr_c2_read(path.encode(), C.c_void_p(iq.ctypes.data), C.byref(freq),
                               C.byref(typ))
    if rc != 0:
        raise N.UwsprError(rc, "cannot read %s" % path)
    return iq, freq.value, typ.value


# ---- transmit side (no device needed up to the symbols) -------------------------------------------------------------
def wspr_pack(text):
    """WSPR message text ("CALL GRID4 dBm", "PFX/CALL dBm", "CALL/SFX dBm", "<CALL> GRID6 dBm") -> the 7 message bytes
    (int8) that unpack_message turns back into text.  Invalid text raises UwsprError (UWSPR_ERR_ARG)."""
    m = np.zeros(7, np.int8)
    rc = N.lib().uwspr_wspr_pack(str(text).encode("ascii", "replace"), C.c_void_p(m.ctypes.data))
    if rc != 0:
        raise N.UwsprError(rc, "not a WSPR message: %r" % (text,))
    return m


def deep_list(known):
    """texts (wspr_pack) or packed messages -> a contiguous [M, 7] int8 array (M = 0: an empty list)"""
    if known is None or len(known) == 0:
        return np.zeros((0, 7), np.int8)
    if isinstance(known, np.ndarray):
        if known.dtype != np.int8 or known.ndim != 2 or known.shape[1] != 7:
            raise TypeError("a list of messages: texts or an [M, 7] int8 array, not %s %s" % (known.dtype, known.shape))
        return np.ascontiguousarray(known)
    return np.ascontiguousarray(np.stack([wspr_pack(t) if isinstance(t, str) else
                                          np.ascontiguousarray(t, dtype=np.int8).reshape(7) for t in known]))


def grid_ngrid(grid4):
    """a 4-character locator -> ngrid, the number uwspr_wspr_pack gives it (0 .. 32399)"""
    g = str(grid4).upper()
    if len(g) != 4 or not ("A" <= g[0] <= "R" and "A" <= g[1] <= "R" and g[2].isdigit() and g[3].isdigit()):
        raise ValueError("a locator is two letters A..R and two digits, not %r" % (grid4,))
    return 180 * (179 - 10 * (ord(g[0]) - 65) - (ord(g[2]) - 48)) + 10 * (ord(g[1]) - 65) + (ord(g[3]) - 48)


def grids_bitmap(grids):
    """2-character fields ("FN": its 100 locators) and / or 4-character locators -> the [4050] uint8 bitmap over ngrid (bit g:
    byte g >> 3, bit g & 7); None: None (every locator)"""
    if grids is None:
        return None
    bm = np.zeros(N.CALL_NGRID // 8, np.uint8)
    for s in ([grids] if isinstance(grids, str) else grids):
        s = str(s)
        if len(s) not in (2, 4):
            raise ValueError("a field (\"FN\") or a locator (\"FN42\"), not %r" % (s,))
        for c in ([s] if len(s) == 4 else ["%s%d%d" % (s, i, j) for i in range(10) for j in range(10)]):
            g = grid_ngrid(c)
            bm[g >> 3] |= 1 << (g & 7)
    return bm


def powers_mask(powers):
    """a subset of native.P19 (dBm) -> the power mask; None: 0 (every power)"""
    if powers is None:
        return 0
    pm = 0
    for p in powers:
        if int(p) != p or int(p) not in N.P19:
            raise N.UwsprError(-6, "call set: %r dBm is not one of the 19 type-1 powers %s" % (p, list(N.P19)))
        pm |= 1 << N.P19.index(int(p))
    if pm == 0:
        raise N.UwsprError(-6, "call set: the set is empty: no power is allowed")
    return pm


def calls_args(calls, grids, powers):
    """-> (char *[A], A, bitmap or None, power mask) for uwspr_calls_set / uwspr_pipe_set_calls"""
    calls = [] if calls is None else ([calls] if isinstance(calls, str) else list(calls))
    arr = (C.c_char_p * max(len(calls), 1))(*[str(c).encode("ascii", "replace") for c in calls])
    return arr, len(calls), grids_bitmap(grids), powers_mask(powers)


def call_message(call, grid4, dbm):
    """message(h): the 7 bytes of "CALL GRID4 dBm" composed from its parts (uwspr_call_message) -- what wspr_pack gives
    for that text"""
    m = np.zeros(7, np.int8)
    rc = N.lib().uwspr_call_message(str(call).encode("ascii", "replace"), grid4 if isinstance(grid4, (int, np.integer)) else grid_ngrid(grid4),
                                    int(dbm), C.c_void_p(m.ctypes.data))
    if rc:
        raise N.UwsprError(rc, "call_message: %r %r %r is not a type-1 message" % (call, grid4, dbm))
    return m


def nhash(key, initval=146):
    """lookup3 hashlittle() of a byte string (the type 3 callsign hash is nhash(call) & 32767)"""
    k = key.encode() if isinstance(key, str) else bytes(key)
    return int(N.lib().uwspr_nhash(k, len(k), int(initval) & 0xFFFFFFFF))


def wspr_symbols(text_or_message):
    """The 162 channel symbols (uint8, 0..3) wsprsim transmits for a message: text, or the 7 bytes of wspr_pack"""
    m = wspr_pack(text_or_message) if isinstance(text_or_message, str) else \
        np.ascontiguousarray(text_or_message, dtype=np.int8).reshape(7)
    sym = np.zeros(N.NSYM, np.uint8)
    N.lib().uwspr_wspr_symbols(C.c_void_p(m.ctypes.data), C.c_void_p(sym.ctypes.data))
    return sym


def write_c2(path, iq, dial_freq=10.1387, type=2):
    """45000 (I,Q) pairs as a .c2 file that c2_read returns unchanged (the file holds Q negated, as wsprsim writes it)"""
    a = np.ascontiguousarray(iq, np.float32).reshape(-1, 2)
    rc = N.lib().uwspr_c2_write(str(path).encode(), C.c_void_p(a.ctypes.data), a.shape[0], float(dial_freq), int(type))
    if rc != 0:
        raise N.UwsprError(rc, "cannot write %s (%d samples; a .c2 file holds 45000)" % (path, a.shape[0]))


def sub_items(items):
    """Subtraction items (Context.subtract) -> a SUB_ITEM_DTYPE array; arrays of that dtype pass through."""
    if isinstance(items, np.ndarray) and items.dtype == N.SUB_ITEM_DTYPE:
        return np.ascontiguousarray(items)
    items = list(items)
    arr = np.zeros(len(items), N.SUB_ITEM_DTYPE)
    for i, s in enumerate(items):
        arr[i]["frame"] = int(s["frame"])
        arr[i]["shift"] = int(s["shift"])
        arr[i]["f_hz"] = float(s["f"])
        arr[i]["drift_hz"] = float(s.get("drift", 0.0))
        sym = s["symbols"] if "symbols" in s else wspr_symbols(s["text"] if "text" in s else s["message"])
        arr[i]["symbols"] = np.asarray(sym, np.uint8).reshape(N.NSYM)
    return arr


def block_items(items):
    """Block-demodulation items (Context.blockdemod) -> a BLOCK_ITEM_DTYPE array; arrays of that dtype pass through."""
    if isinstance(items, np.ndarray) and items.dtype == N.BLOCK_ITEM_DTYPE:
        return np.ascontiguousarray(items)
    items = list(items)
    arr = np.zeros(len(items), N.BLOCK_ITEM_DTYPE)
    for i, s in enumerate(items):
        arr[i]["frame"] = int(s["frame"])
        arr[i]["shift"] = int(s["shift"])
        arr[i]["f_hz"] = float(s["f"])
        arr[i]["drift_hz"] = float(s.get("drift", 0.0))
    return arr


def tx_signals(signals):
    """A list of transmissions -> the uwspr_tx_signal array.  Each is a dict: "text" (or "message": 7 bytes, or
    "symbols": 162), "channel" (0), "start" (baseband sample of the first symbol, 375), "f0" (Hz, 0), "drift" (Hz over the
    transmission, 0), "phase0" (rad, 0), "gain" (1), and optionally "motion" (tx_motions) and "carrier" (tx_carriers)."""
    signals = list(signals)
    arr = (N.TxSignal * max(len(signals), 1))()
    for i, s in enumerate(signals):
        if "symbols" in s:
            sym = np.asarray(s["symbols"], np.uint8).reshape(N.NSYM)
        else:
            sym = wspr_symbols(s["text"] if "text" in s else s["message"])
        C.memmove(arr[i].symbols, sym.ctypes.data, N.NSYM)
        arr[i].channel = int(s.get("channel", 0))
        arr[i].start = int(s.get("start", 375))
        arr[i].f0_hz, arr[i].drift_hz = float(s.get("f0", 0.0)), float(s.get("drift", 0.0))
        arr[i].phase0, arr[i].gain = float(s.get("phase0", 0.0)), float(s.get("gain", 1.0))
    return arr if signals else (N.TxSignal * 0)()


def tx_carriers(signals):
    """The carrier array (int32, Hz) of a list of transmissions (tx_signals' dicts), or None when none has a "carrier":
    the calls then go the way they always went.  A signal without the key stays at 1500 Hz."""
    signals = list(signals)
    if not any("carrier" in s for s in signals):
        return None
    out = np.empty(len(signals), np.int32)
    for i, s in enumerate(signals):
        fc = s.get("carrier", 1500)
        if int(fc) != fc:
            raise ValueError("carrier: integer Hz, not %r" % (fc,))
        out[i] = int(fc)
    return out


def tx_fades(signals):
    """The uwspr_tx_fade array of a list of transmissions (tx_signals' dicts), or None when none has a "fading".  A fading
    is a dict: "spread" (Hz: the Doppler spread, two sigma of a Gaussian Doppler spectrum, 0 .. 20), "shift" (Hz, the
    scattered part's mean Doppler, 0), "k" (the Rician K factor, fixed : scattered power, 0 = Rayleigh), "seed" (0) and
    "paths" (the sinusoids summed, 16; 1 with k = 0 is a pure Doppler shift).  A signal without one does not fade
    (paths = 0).  include/uwspr_hip.h states the model."""
    signals = list(signals)
    if not any(s.get("fading") is not None for s in signals):
        return None
    arr = (N.TxFade * len(signals))()
    for i, s in enumerate(signals):
        f = s.get("fading")
        if f is None:
            continue
        unknown = set(f) - {"spread", "shift", "k", "seed", "paths"}
        if unknown:
            raise ValueError("fading: unknown keys %s" % sorted(unknown))
        arr[i].spread_hz, arr[i].shift_hz, arr[i].k_factor = float(f["spread"]), float(f.get("shift", 0.0)), float(f.get("k", 0.0))
        arr[i].seed, arr[i].paths = int(f.get("seed", 0)) & (2 ** 64 - 1), int(f.get("paths", 16))
    return arr


def tx_impulses(impulses, channels):
    """The uwspr_tx_impulse array of tx_render's `impulses` (None; one dict for every channel; or a list of one dict or
    None per channel), or None when there are none.  Keys: "rate", "sigma", "seed" (0), "length" (1)."""
    if impulses is None:
        return None
    per = list(impulses) if isinstance(impulses, (list, tuple)) else [impulses] * channels
    if len(per) != channels:
        raise ValueError("impulses: %d entries for %d channels" % (len(per), channels))
    if all(z is None for z in per):
        return None
    arr = (N.TxImpulse * max(channels, 1))()
    for k, z in enumerate(per):
        arr[k].length = 1
        if z is None:
            continue
        unknown = set(z) - {"rate", "sigma", "seed", "length"}
        if unknown:
            raise ValueError("impulses: unknown keys %s" % sorted(unknown))
        arr[k].rate, arr[k].sigma = float(z["rate"]), float(z["sigma"])
        arr[k].seed, arr[k].length = int(z.get("seed", 0)) & (2 ** 64 - 1), int(z.get("length", 1))
    return arr


_TX_MODELS = {"static": N.TX_STATIC, "doppler": N.TX_DOPPLER, "delay": N.TX_DELAY}


def tx_motions(signals):
    """The uwspr_tx_motion array of a list of transmissions (tx_signals' dicts), or None when none has a "motion".  A
    motion is a dict: "v" (V1, V2) m/s, "p" (p1, p2) m (the source at (V1 t + p1, V2 t + p2), the hydrophone at the
    origin: slm.cc's straight-line model), "t" (trajectory time of the transmission's first sample, s, 0), "model"
    ("doppler": the carrier Doppler alone, the receiver's model; "delay": propagation delay as well; "static"),
    "absolute" (False: delay and phase relative to R(t_first); True: R / c, `start` being the emission time) and
    "spreading" (False; True: amplitude R(t_first) / R(t)).  include/uwspr_hip.h states the model."""
    signals = list(signals)
    if not any(s.get("motion") is not None for s in signals):
        return None
    arr = (N.TxMotion * len(signals))()
    for i, s in enumerate(signals):
        m = s.get("motion")
        if m is None:
            continue
        unknown = set(m) - {"v", "p", "t", "model", "absolute", "spreading"}
        if unknown:
            raise ValueError("motion: unknown keys %s" % sorted(unknown))
        v, p = m.get("v", (0.0, 0.0)), m.get("p", (0.0, 0.0))
        arr[i].v1, arr[i].v2 = float(v[0]), float(v[1])
        arr[i].p1, arr[i].p2 = float(p[0]), float(p[1])
        arr[i].t_first = float(m.get("t", 0.0))
        model = m.get("model", "doppler")
        arr[i].model = _TX_MODELS[model] if isinstance(model, str) else int(model)
        arr[i].flags = (N.TX_ABSOLUTE if m.get("absolute", False) else 0) | (N.TX_SPREADING if m.get("spreading", False) else 0)
    return arr


def slm_trajectories():
    """The receiver's 125 straight-line-model trajectories, [125, 4] float64 (V1, V2, p1, p2), in slmGenerator's order
    (lib/slm.cc:76-116): p2 = 50 .. 850 step 200 fastest, then V1 = -2 .. 2, then V2 = -2 .. 2 (m/s); p1 = 0."""
    out = np.zeros((125, 4), np.float64)
    i = 0
    for v2 in range(-2, 3):
        for v1 in range(-2, 3):
            for p2 in range(50, 851, 200):
                out[i] = (v1, v2, 0.0, p2)
                i += 1
    return out


def slm_drift(traj, t, cf=1500.0):
    """The straight-line-model Doppler in Hz, binary64: slmFrequencyDrift (lib/slm.cc:36-73) = -(cf / c) dR/dt with
    R(t) = |(V1 t + p1, V2 t + p2)| and c = 1500 m/s (0 where R = 0).  traj: (V1, V2, p1, p2) or an [..., 4] array; t in
    seconds; the result broadcasts traj[..., 0] against t."""
    a = np.asarray(traj, np.float64)
    V1, V2, p1, p2 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    t = np.asarray(t, np.float64)
    q1, q2 = V1 * t + p1, V2 * t + p2
    R = np.hypot(q1, q2)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(R > 0, -(V1 * q1 + V2 * q2) / np.where(R > 0, R, 1.0) * (float(cf) / 1500.0), 0.0)
    return d


def _track_model(model):
    return _TX_MODELS[model] if isinstance(model, str) else int(model)


def track_trajs(trajs):
    """Trajectories (v m/s, d m, tc s) -> a TRACK_TRAJ_DTYPE array: arrays of that dtype pass through; else (v, d, tc)
    tuples, dicts with those keys, or an [n, 3] array."""
    if isinstance(trajs, np.ndarray) and trajs.dtype == N.TRACK_TRAJ_DTYPE:
        return np.ascontiguousarray(trajs).reshape(-1)
    if isinstance(trajs, dict):
        trajs = [trajs]
    rows = [(t["v"], t["d"], t["tc"]) if isinstance(t, dict) else tuple(t) for t in (trajs.tolist() if isinstance(trajs, np.ndarray) else list(trajs))]
    out = np.zeros(len(rows), N.TRACK_TRAJ_DTYPE)
    for i, r in enumerate(rows):
        if len(r) != 3:
            raise ValueError("trajectory %d: (v, d, tc), not %r" % (i, r))
        out[i] = tuple(float(x) for x in r)
    return out


def track_grid(v, d, tc):
    """The product grid of speeds v (m/s), CPA ranges d (m) and CPA times tc (s from the item's first sample) -> a
    TRACK_TRAJ_DTYPE array, v slowest and tc fastest.  A source at rest has neither a CPA range nor a CPA time that matter:
    v = 0 gives the single entry (0, d[0], 0)."""
    v, d, tc = (np.atleast_1d(np.asarray(a, np.float64)) for a in (v, d, tc))
    if not (v.size and d.size and tc.size):
        raise ValueError("track_grid: v, d and tc need at least one value each")
    rows = []
    for a in v:
        if a == 0.0:
            rows.append((0.0, float(d[0]), 0.0))
        else:
            rows += [(float(a), float(b), float(c)) for b in d for c in tc]
    if len(rows) > N.TRACK_MAX:
        raise ValueError("track_grid: %d trajectories, a set holds at most %d" % (len(rows), N.TRACK_MAX))
    return track_trajs(rows)


def track_from_slm(traj, t_first=0.0):
    """Straight-line-model parameters (V1, V2, p1, p2), or an [n, 4] array of them (slm_trajectories), with the trajectory
    time t_first of the item's first sample -> the (v, d, tc) of uwspr_track_from_slm, a TRACK_TRAJ_DTYPE array [n]."""
    a = np.asarray(traj, np.float64).reshape(-1, 4)
    out = np.zeros(len(a), N.TRACK_TRAJ_DTYPE)
    L = N.lib()
    for i, (v1, v2, p1, p2) in enumerate(a):
        rc = L.uwspr_track_from_slm(float(v1), float(v2), float(p1), float(p2), float(t_first), C.c_void_p(out[i:i + 1].ctypes.data))
        if rc != 0:
            raise N.UwsprError(rc, "track_from_slm: non-finite parameters %r" % ((v1, v2, p1, p2, t_first),))
    return out


def track_doppler(traj, t, cf=1500.0):
    """The Doppler in Hz of trajectories (track_trajs) at times t (s from the item's first sample), binary64:
    -(cf / c) Rdot(t) with R(t) = sqrt(d^2 + (v (t - tc))^2), c = 1500 m/s (0 where R = 0) -> [n, len(t)], or [len(t)] for
    one trajectory given as a tuple or dict."""
    one = isinstance(traj, (tuple, dict)) or (isinstance(traj, np.ndarray) and traj.dtype == N.TRACK_TRAJ_DTYPE and traj.ndim == 0)
    tr = track_trajs([traj] if one else traj)
    t = np.atleast_1d(np.asarray(t, np.float64))
    a = tr["v"][:, None] * (t[None, :] - tr["tc"][:, None])
    R = np.sqrt(tr["d"][:, None] * tr["d"][:, None] + a * a)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(R > 0, -(float(cf) / 1500.0) * ((tr["v"][:, None] * a) / np.where(R > 0, R, 1.0)), 0.0)
    return out[0] if one else out


def track_design(trajs, model="delay", cf=1500.0):
    """uwspr_track_design: the per-symbol tables of trajectories (track_trajs) -> (dfreq [n, 162] float64 Hz relative to
    mid-transmission, tau [n, 162] int32 samples; all zero for model "doppler")."""
    tr = track_trajs(trajs)
    df, ta = np.zeros((len(tr), N.NSYM), np.float64), np.zeros((len(tr), N.NSYM), np.int32)
    rc = N.lib().uwspr_track_design(C.c_void_p(tr.ctypes.data) if len(tr) else None, len(tr), _track_model(model), float(cf),
                                    C.c_void_p(df.ctypes.data), C.c_void_p(ta.ctypes.data))
    if rc != 0:
        raise N.UwsprError(rc, "track_design: trajectories outside 0 <= v <= 10, 1 <= d <= 1e6, |tc| <= 1e4, an unknown model or a bad cf")
    return df, ta


def track_motion(traj, bearing=0.0, model="delay"):
    """A (v, d, tc) trajectory as a "motion" dict of tx_signals, so that what Context.track fits can be rendered: the CPA
    lies at range d in direction `bearing` (rad; the fit cannot see it) and the source passes it at right angles;
    trajectory time 0 is the transmission's first sample."""
    tr = track_trajs([traj])[0]
    v, d, tc = float(tr["v"]), float(tr["d"]), float(tr["tc"])
    cb, sb = float(np.cos(bearing)), float(np.sin(bearing))
    V = (-v * sb, v * cb)
    return {"v": V, "p": (d * cb - V[0] * tc, d * sb - V[1] * tc), "t": 0.0, "model": model}


def tx_sigma(snr_db, gain=1.0):
    """AWGN sigma (per 12 kS/s audio sample) that puts a transmission of baseband amplitude `gain` at snr_db in 2500 Hz
    at the transmit chain's output: the chain makes it a real tone of amplitude gain / 32 (the interpolation filter has
    unit gain), of power (gain / 32)^2 / 2 against sigma^2 2500 / 6000 of noise in 2500 Hz."""
    a = float(gain) / 32.0
    return float(np.sqrt(0.5 * a * a * (AUDIO_RATE / 2.0) / 2500.0 * 10.0 ** (-float(snr_db) / 10.0)))


def encode_wav(path, schedule, channels=1, snr_db=None, seed=0, gain=1.0, seconds=None, piece_s=60, ctx=None, impulses=None):
    """c2ToWaveFile from text: a 16-bit 12 kS/s WAV of `channels` channels carrying the schedule's transmissions.
    schedule: (text, channel, start_s, f0) entries; start_s is the start of the entry's 2-minute slot (its first symbol
    is 1 s later, as in a .c2 file) and f0 the offset in Hz (the transmission is centred on 1500 + f0 Hz).  An entry may
    also be a tx_signals dict (a moving source: its "motion"; another carrier: its "carrier" in Hz, the transmission then
    centred on carrier + f0 -- what decode_wav(carriers=[...]) listens to), its gain `gain` unless it names one.  snr_db: AWGN per channel (seed + channel) for that SNR in 2500 Hz, None = none.  The file is rendered
    in pieces of piece_s seconds and lasts `seconds` (default: until the last slot's frame is complete).  A dict entry may
    carry a "fading" (tx_fades); impulses: tx_render's (impulsive noise per channel)."""
    import wave
    sig, slots = [], []
    for e in schedule:
        if isinstance(e, dict):
            sig.append(dict({"gain": gain}, **e))
            slots.append((int(e.get("start", 375)) - 375) / 375.0)
        else:
            t, c, s0, f0 = e
            sig.append({"text": t, "channel": int(c), "start": int(round(375 * float(s0))) + 375, "f0": float(f0), "gain": gain})
            slots.append(float(s0))
    if seconds is None:
        seconds = max(slots + [0.0]) + 121.0
    n = int(round(seconds * AUDIO_RATE))
    own = ctx is None
    ctx = Context() if own else ctx
    sigma = 0.0 if snr_db is None else tx_sigma(snr_db, gain)
    try:
        with wave.open(str(path), "wb") as w:
            w.setnchannels(int(channels))
            w.setsampwidth(2)
            w.setframerate(AUDIO_RATE)
            step = int(piece_s * AUDIO_RATE)
            for k in range(0, n, step):
                x = ctx.tx_render(sig, min(step, n - k), t0=k, channels=channels, sigma=sigma,
                                  seed=[int(seed) + c for c in range(int(channels))], format="s16", impulses=impulses)
                w.writeframes(x.astype("<i2").tobytes())
    finally:
        if own:
            ctx.close()


class Pipe:
    """uwspr_pipe_*: the pipelined end-to-end decoder (stream ingest on a copy stream, lazy schedule,
    Fano on the persistent host pool under the next batch's kernels, resume of what try 0 did not
    decode).  Results are DECODE_DTYPE records in frame order."""

    def __init__(self, fs=375, fl=45000, spb=256, maxdrift=0, maxfreqs=200, halfbandwidth=10, cf=1500,
                 threshold=10, device=0, hop=3375, batch_frames=256, max_per_frame=1, lanes=0,
                 host_threads=0, eager=False, sched=None, spare_after_us=0, passes=1, osd=0, osd_gap=None,
                 block=0, audio_rate=None, blank=0, blank_guard=None, carriers=None, frontend_hbw=None, known=None,
                 deep_min=None, deep_gap=None, calls=None, call_grids=None, call_powers=None, call_min=None, call_gap=None,
                 tracks=None, track_qf=4, track_model="delay", follow=None, follow_qf=8, follow_lags=1, follow_model="doppler"):
        self.L = N.lib()
        self.carriers = [1500]
        self.track_trajs, self.track_nf, self.track_qf = None, 1, 0
        self.follow_trajs, self.follow_nf, self.follow_qf, self.follow_nl = None, 1, 0, 0
        self.h = C.c_void_p()
        self.fl = fl
        p = N.Params(fs, fl, spb, maxdrift, maxfreqs, halfbandwidth, cf, threshold)
        o = N.PipeOpts(hop, batch_frames, max_per_frame, lanes, host_threads, 1 if eager else 0,
                       {None: 0, "fused": 1, "staged": 2}[sched], int(spare_after_us))
        rc = self.L.uwspr_pipe_open(C.byref(p), device, C.byref(o), C.byref(self.h))
        if rc != 0:
            msg = self.L.uwspr_pipe_last_error(self.h).decode() if self.h else ""
            if self.h:
                self.L.uwspr_pipe_close(self.h)
            self.h = None
            raise N.UwsprError(rc, msg)
        self.batch_frames, self.hop = batch_frames, hop
        def options(*rows):   # (keyword's value, option, whether to set it), in order
            for value, name, wanted in rows:
                if wanted:
                    self.set_option(name, value)
        try:   # in this order: the carriers before frontend_hbw, a list before its thresholds
            options((passes, "passes", passes != 1),   # 2: what decodes is subtracted and the residual searched again (records with pass = 1)
                    (osd, "osd", osd),                 # 1, 2: ordered-statistics decoding of that order on what Fano timed out on (records with osd = 1)
                    (osd_gap, "osd_gap", osd_gap is not None),
                    (block, "block", block),           # 2, 3: block demodulation up to that length on what Fano timed out on (records with block = 2, 3)
                    # push_audio takes audio at that rate (K11 ahead of the front-end)
                    (audio_rate, "audio_rate", audio_rate is not None and int(audio_rate) != AUDIO_RATE),
                    (blank, "blank", blank),           # 4 .. 1024: the noise blanker K12 ahead of everything push_audio feeds, threshold blank / 4 block medians
                    (blank_guard, "blank_guard", blank_guard is not None))
            if carriers is not None:   # K0's centres in Hz: every pushed channel is heard at every one of them
                self.set_carriers(carriers)
            options((frontend_hbw, "frontend_hbw", frontend_hbw is not None))
            if known is not None and len(known):   # the list of expected messages: K13 on what Fano timed out on (records with osd = 2)
                self.set_list(known)
            options((deep_min, "deep_min", deep_min is not None), (deep_gap, "deep_gap", deep_gap is not None))
            if calls is not None and len(calls):   # the call set: K14 on what Fano timed out on and the list left (records with osd = 3)
                self.set_calls(calls, call_grids, call_powers)
            options((call_min, "call_min", call_min is not None), (call_gap, "call_gap", call_gap is not None))
            if tracks is not None and len(tracks):   # the trajectory set: K15 on every decoded record (tracks())
                self.set_tracks(tracks, track_qf, track_model)
            if follow is not None and len(follow):   # the follow set: K16 on what Fano timed out on (records with osd = 4, follows())
                self.set_follow(follow, follow_qf, follow_lags, follow_model)
        except N.UwsprError:
            self.close()
            raise

    def _chk(self, rc):
        if rc < 0:
            raise N.UwsprError(rc, self.L.uwspr_pipe_last_error(self.h).decode())
        return rc

    def close(self):
        if self.h:
            self.L.uwspr_pipe_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def push(self, iq):
        a = np.ascontiguousarray(iq, np.float32)
        self._chk(self.L.uwspr_pipe_push(self.h, C.c_void_p(a.ctypes.data), a.size // 2))

    def push_audio(self, x):
        """Real audio at the pipe's audio_rate (default 12 kS/s): a 1-D numpy float32 or int16 array of any length
        (uwspr_pipe_push_audio), or a 2-D [n, C] one of C interleaved channels (uwspr_pipe_push_audio_channels; the
        first push fixes C)"""
        a = np.asarray(x)
        if a.ndim == 2:
            if a.dtype not in (np.float32, np.int16):
                raise TypeError("audio: a [n, C] float32 or int16 array, not %s %s" % (a.dtype, a.shape))
            a = np.ascontiguousarray(a)
            self._chk(self.L.uwspr_pipe_push_audio_channels(self.h, C.c_void_p(a.ctypes.data), a.shape[0], a.shape[1],
                                                            _audio_format(a)))
            return
        a = _audio_array(a)
        self._chk(self.L.uwspr_pipe_push_audio(self.h, C.c_void_p(a.ctypes.data), a.size, _audio_format(a)))

    def acquire(self, nsamples):
        """-> numpy view [nsamples, 2] of the page-locked staging buffer to fill; then commit(nsamples)."""
        ptr = C.c_void_p()
        self._chk(self.L.uwspr_pipe_acquire(self.h, int(nsamples), C.byref(ptr)))
        buf = (C.c_float * (2 * int(nsamples))).from_address(ptr.value)
        return np.frombuffer(buf, np.float32).reshape(-1, 2)

    def commit(self, nsamples):
        self._chk(self.L.uwspr_pipe_commit(self.h, int(nsamples)))

    def submit_device(self, frames, B=None, stride=0):
        """frames: torch CUDA tensor [B, fl, 2] (or a raw pointer with B given)."""
        if _is_torch(frames):
            B = frames.numel() // (2 * self.fl) if B is None else B
            ptr = frames.data_ptr()
        else:
            ptr = int(frames)
        self._chk(self.L.uwspr_pipe_submit_device(self.h, C.c_void_p(ptr), int(B), int(stride)))

    def flush(self):
        self._chk(self.L.uwspr_pipe_flush(self.h))

    def collect(self, cap=65536, wait=False):
        out = np.zeros(cap, N.DECODE_DTYPE)
        n = self._chk(self.L.uwspr_pipe_collect(self.h, C.c_void_p(out.ctypes.data), cap, 1 if wait else 0))
        return out[:n].copy()

    def inject_failure(self, batch, where):
        """test hook: batch number `batch` fails at its launch (where = 0) or in its host tail (where = 1)"""
        self._chk(self.L.uwspr_pipe_inject_failure(self.h, int(batch), int(where)))

    def set_option(self, name, value):
        """uwspr_pipe_set_option: an option of every lane's context; only while nothing is in flight"""
        self._chk(self.L.uwspr_pipe_set_option(self.h, name.encode(), int(value)))

    def set_list(self, known):
        """uwspr_pipe_set_list: the list of expected messages (texts or an [M, 7] int8 array; empty: the stage is off);
        only while nothing is in flight"""
        m = deep_list(known)
        self._chk(self.L.uwspr_pipe_set_list(self.h, C.c_void_p(m.ctypes.data) if len(m) else None, len(m)))

    def set_calls(self, calls, grids=None, powers=None):
        """uwspr_pipe_set_calls: the call set (callsigns, grids and powers as at Context.calls_set; no callsign: the stage
        is off); only while nothing is in flight"""
        arr, A, bm, pm = calls_args(calls, grids, powers)
        self._chk(self.L.uwspr_pipe_set_calls(self.h, arr, A, C.c_void_p(bm.ctypes.data) if bm is not None else None, pm))

    def set_tracks(self, trajs, qf=4, model="delay"):
        """uwspr_pipe_set_tracks: the trajectory set (as at Context.track_set; empty: the stage is off); only while nothing is
        in flight"""
        tr = track_trajs(trajs if trajs is not None else [])
        self._chk(self.L.uwspr_pipe_set_tracks(self.h, C.c_void_p(tr.ctypes.data) if len(tr) else None, len(tr), int(qf), _track_model(model)))
        self.track_trajs, self.track_qf, self.track_nf = (tr, int(qf), 2 * int(qf) + 1) if len(tr) else (None, 0, 1)

    def tracks(self, cap=65536):
        """uwspr_pipe_collect_tracks: the trajectory fits of the decoded records emitted so far (never waits), a
        TRACK_RECORD_DTYPE array in the order of the decoded records: frame, cand, channel, pass and result (best, t_best,
        t_ref, f_hz); track_of gives a record's (v, d, tc)."""
        out = np.zeros(cap, N.TRACK_RECORD_DTYPE)
        n = self._chk(self.L.uwspr_pipe_collect_tracks(self.h, C.c_void_p(out.ctypes.data), cap))
        return out[:n].copy()

    def track_of(self, rec):
        """a track record -> the "track" dict of decode_wav: v, d, tc of the best trajectory, the fitted f, t_best, t_ref"""
        r = rec["result"]
        t = self.track_trajs[int(r["best"]) // self.track_nf]
        return {"v": float(t["v"]), "d": float(t["d"]), "tc": float(t["tc"]), "f": float(r["f_hz"]),
                "t_best": float(r["t_best"]), "t_ref": float(r["t_ref"])}

    def set_follow(self, grid, qf=8, lags=1, model="doppler"):
        """uwspr_pipe_set_follow: the follow set (as at Context.follow_set; empty: the stage is off); only while nothing is in
        flight"""
        tr = track_trajs(grid if grid is not None else [])
        self._chk(self.L.uwspr_pipe_set_follow(self.h, C.c_void_p(tr.ctypes.data) if len(tr) else None, len(tr), int(qf), int(lags),
                                               _track_model(model)))
        self.follow_trajs, self.follow_qf, self.follow_nf, self.follow_nl = (tr, int(qf), 2 * int(qf) + 1, int(lags)) if len(tr) else (None, 0, 1, 0)

    def follows(self, cap=65536):
        """uwspr_pipe_collect_follows: the fits of the records K16 decoded (osd = 4) emitted so far (never waits), a
        FOLLOW_RECORD_DTYPE array in the order of those records: frame, cand, channel, pass and result (best, s_best, s_ref,
        f_hz); follow_of gives a record's pass, frequency and lag."""
        out = np.zeros(cap, N.FOLLOW_RECORD_DTYPE)
        n = self._chk(self.L.uwspr_pipe_collect_follows(self.h, C.c_void_p(out.ctypes.data), cap))
        return out[:n].copy()

    def follow_of(self, rec):
        """a follow record -> the "follow" dict of decode_wav: v, d, tc of the best pass, the fitted f, the lag in samples,
        s_best, s_ref"""
        r = rec["result"]
        nlg = 2 * self.follow_nl + 1
        t = self.follow_trajs[int(r["best"]) // (self.follow_nf * nlg)]
        return {"v": float(t["v"]), "d": float(t["d"]), "tc": float(t["tc"]), "f": float(r["f_hz"]),
                "lag": N.FOLLOW_LSTEP * (int(r["best"]) % nlg - self.follow_nl), "s_best": float(r["s_best"]), "s_ref": float(r["s_ref"])}

    def set_carriers(self, hz):
        """uwspr_pipe_set_carriers: K0's centres in Hz (distinct integers, order kept), before the first audio push.  With
        more than one, a record's "channel" field is the plane index: split_plane gives (channel, carrier)."""
        car = np.ascontiguousarray([int(v) for v in hz], np.int32).reshape(-1)
        self._chk(self.L.uwspr_pipe_set_carriers(self.h, C.c_void_p(car.ctypes.data), int(car.size)))
        self.carriers = [int(v) for v in car]

    def split_plane(self, channel_field):
        """a record's "channel" field -> (audio channel, carrier in Hz): the field holds channel * n + k with n carriers"""
        n = len(self.carriers)
        return int(channel_field) // n, self.carriers[int(channel_field) % n]

    def blank_stats(self, channels=1):
        """uwspr_pipe_blank_stats: per channel, (samples output, samples set to zero) by the pipe's blanker -> two int64
        arrays [channels]; zeros when the pipe's "blank" is 0"""
        s, z = np.zeros(int(channels), np.int64), np.zeros(int(channels), np.int64)
        self._chk(self.L.uwspr_pipe_blank_stats(self.h, C.c_void_p(s.ctypes.data), C.c_void_p(z.ctypes.data), int(channels)))
        return s, z

    def stats(self):
        st = N.PipeStats()
        self._chk(self.L.uwspr_pipe_get_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in N.PipeStats._fields_}


# ---- recordings ---------------------------------------------------------------------------------------------------
def supported_rate(rate):
    """whether the resampler takes audio at `rate` S/s (include/uwspr_hip.h; 12000 = no resampler)"""
    rate = int(rate)
    return 8000 <= rate <= 192000 and AUDIO_RATE // int(np.gcd(rate, AUDIO_RATE)) <= 160


def read_wav(path, channels=None, any_rate=False):
    """A 16-bit PCM WAV (stdlib wave) -> (channel 0 as int16, rate); channels="all": ([n, C] int16, rate), every
    channel.  Anything else -- another sample width, a float WAV, a rate other than the front-end's 12000 S/s --
    raises ValueError.  any_rate=True: every rate the resampler supports (Pipe(audio_rate=rate) takes it); ValueError
    naming the rate otherwise."""
    if channels not in (None, "all"):
        raise ValueError("read_wav: channels=None (channel 0) or \"all\", not %r" % (channels,))
    import wave
    try:
        w = wave.open(str(path), "rb")
    except wave.Error as e:   # e.g. "unknown format: 3" = IEEE float
        raise ValueError("%s: not a 16-bit PCM WAV (%s)" % (path, e)) from None
    with w:
        width, nch, rate, n = w.getsampwidth(), w.getnchannels(), w.getframerate(), w.getnframes()
        if width != 2:
            raise ValueError("%s: %d-bit samples; 16-bit PCM only" % (path, 8 * width))
        if any_rate and not supported_rate(rate):
            raise ValueError("%s: %d S/s is not a supported rate (8000 .. 192000 S/s with 12000 / gcd(rate, 12000) <= 160)" % (path, rate))
        if rate != AUDIO_RATE and not any_rate:
            raise ValueError("%s: %d S/s; the front-end takes %d S/s" % (path, rate, AUDIO_RATE))
        raw = w.readframes(n)
    x = np.frombuffer(raw, dtype="<i2").reshape(-1, nch)
    if channels is None:
        x = x[:, 0]
    return np.ascontiguousarray(x, dtype=np.int16), rate


def record_dict(r):
    """a decoded pipe record -> decode_wav's dict without its "channel" and "carrier" (the record's osd byte split into
    "osd", "deep" and "call")"""
    return {"frame": int(r["frame"]), "t": int(r["stream_pos"]) / 375.0,
            "freq": float(r["coarse"]["freq"]), "snr": float(r["coarse"]["snr"]),
            "text": unpack_message(r["message"])[1], "pass": int(r["pass"]), "osd": int(r["osd"] == 1),
            "block": int(r["block"]), "deep": int(r["osd"] == 2), "call": int(r["osd"] == 3)}


def decode_wav(path, channels=None, **pipe_opts):
    """Decode a recording (12 kS/s, or any rate read_wav(any_rate=True) returns: the pipe's audio_rate is set from the
    file) as the receiver flowgraph does (examples/AudioSourceDecode.grc): the file through a
    Pipe's push_audio -> one dict per decoded record, in frame order: frame, t (stream_pos / 375 s), the coarse freq
    and snr, the unpacked text, "pass" (1: found by the second pass of passes=2, under a decoded signal; else 0) and
    "osd" (1: Fano timed out and ordered-statistics decoding gave the message, osd=1 or 2; else 0) and "block" (2, 3: Fano
    timed out and the soft symbols coherent over that many symbols decoded, block=2 or 3; else 0) and "deep" (1: Fano timed
    out and the list search gave the message, known=[texts or packed messages]; else 0) and "call" (1: Fano timed out and
    the call search gave the message, calls=[callsigns]; else 0).
    channels="all": every channel of the file through one pipe, records in (take, channel, frame) order, each dict with
    its "channel".  carriers=[Hz, ..]: every channel is heard at each of them (Pipe(carriers=..)), records in (take,
    channel, carrier, frame) order, each dict with its "carrier" in Hz ("channel" stays the audio channel).
    tracks=grid (track_grid; with track_qf, track_model): every decoded dict gets a "track" dict -- v, d, tc of the best
    straight-line pass, the fitted f, t_best and t_ref (Context.track states them).
    follow=grid (with follow_qf, follow_lags, follow_model): what Fano times out on is demodulated along the grid's passes
    (K16), and every decoded dict gets "follow": v, d, tc of the pass, the fitted f, the lag in samples, s_best and s_ref for a
    record K16 decoded, None for every other."""
    x, rate = read_wav(path, channels, any_rate=True)
    carriers = pipe_opts.get("carriers")
    pipe = Pipe(audio_rate=rate, **pipe_opts)
    try:
        piece = rate * 60
        for k in range(0, x.shape[0], piece):
            pipe.push_audio(x[k:k + piece])
        pipe.flush()
        recs = pipe.collect(cap=1 << 20)
        fits = pipe.tracks(cap=1 << 20) if pipe.track_trajs is not None else None
        ffits = pipe.follows(cap=1 << 20) if pipe.follow_trajs is not None else None
        nfol = 0
    finally:
        pipe.close()
    out = []
    for r in recs:
        if not r["decoded"]:
            continue
        d = record_dict(r)
        if fits is not None:   # one per decoded record, in their order
            d["track"] = pipe.track_of(fits[len(out)])
        if ffits is not None:   # one per record K16 decoded, in their order
            d["follow"] = pipe.follow_of(ffits[nfol]) if r["osd"] == 4 else None
            nfol += int(r["osd"] == 4)
        ch, car = pipe.split_plane(r["channel"])
        if channels == "all":
            d["channel"] = ch
        if carriers is not None:
            d["carrier"] = car
        out.append(d)
    return out
