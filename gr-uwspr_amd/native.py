"""Build + ctypes binding of libuwspr_hip.so (include/uwspr_hip.h).

This module is plumbing only: it compiles the HIP sources for gfx950 in-tree
and maps the C ABI one-to-one.  There is no Python or CPU implementation of the
path behind it: if the library cannot be built or loaded, or no gfx950 device
is present, calls raise UwsprError.
"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIBDIR = os.path.join(_HERE, "lib")
# An experiment build (UWSPR_EXTRA_HIPFLAGS set: extra compiler flags for an A/B) goes to its OWN
# library file, so the product libuwspr_hip.so is never replaced by a build whose results may be
# invalid; with the variable unset the product library is (re)built from the default flags.
_EXTRA = os.environ.get("UWSPR_EXTRA_HIPFLAGS", "").replace(",", " ").split()   # (commas: for shell A/B scripts)
# (one file per flag set, so that interleaved A/B runs do not rebuild each other's library)
_EXTRA_TAG = hashlib.sha256(" ".join(_EXTRA).encode()).hexdigest()[:8] if _EXTRA else ""
LIBPATH = os.path.join(LIBDIR, "libuwspr_hip_exp_%s.so" % _EXTRA_TAG if _EXTRA else "libuwspr_hip.so")
HOSTLIB = os.path.join(LIBDIR, "libuwspr_blocks.so")

SOURCES = ["uwspr_api.hip", "k0_frontend.hip", "k1_spectrogram.hip", "k2_spectrum.hip", "k3_coarse.hip",
           "k4_tonecorr.hip", "k4_grid.hip", "k4_pair.hip", "k4_jig.hip", "k5_fold_schedule.hip", "k6_sched.hip", "k7_transmit.hip", "k8_subtract.hip", "k9_osd.hip", "k10_blockdemod.hip", "k11_resample.hip", "k12_blank.hip", "k13_deep.hip", "k14_calls.hip", "k15_track.hip", "k16_follow.hip", "pipe.hip", "dist.hip", "host_tail.cpp"]
HIPFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
            "-fno-slp-vectorize", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fPIC", "-Wall", "-Wno-unused-function"]

NSYM, NSLM, NK0, NIFR, NJIG = 162, 125, 26, 5, 17
HOST, DEVICE, DEVICE_FRAMES, HOST_ASYNC = 0, 1, 2, 3
AUDIO_F32, AUDIO_S16 = 0, 1
LINEAR, NONLINEAR = 0, 1


class UwsprError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("uwspr status %d: %s" % (status, msg))
        self.status = status


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise UwsprError(-4, "hipcc not found")


def _compiler_id():
    """What identifies the compiler in the build stamp without starting it on every import: the resolved
    path of hipcc, its size and the ROCm release file next to it (another ROCm => another stamp => rebuild).
    "absent" when there is no compiler: a shipped library whose stamp says otherwise is then still used."""
    try:
        cc = os.path.realpath(_hipcc())
    except UwsprError:
        return "hipcc absent"
    ver = ""
    for v in (os.path.join(os.path.dirname(os.path.dirname(cc)), ".info", "version"), "/opt/rocm/.info/version"):
        if os.path.exists(v):
            ver = open(v).read().strip()
            break
    return "%s size %d rocm %s" % (cc, os.path.getsize(cc), ver)


def _digest(paths):
    """Content hash of the build inputs: what decides whether the library is current (file
    times do not survive a copy to another machine; contents do)."""
    h = hashlib.sha256()
    for q in sorted(paths):
        h.update(os.path.basename(q).encode())
        with open(q, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _sources():
    """-> (the sources of the product library, everything its build reads: those, csrc's headers and the ABI header)"""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]
    deps.append(os.path.join(_HERE, "..", "include", "uwspr_hip.h"))
    return srcs, deps


def source_digest():
    """sha256 over the sources the product library is built from (what a profile taken with
    tools/run_profiles.sh is valid for)."""
    return _digest(_sources()[1])


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 every kernel + the C ABI into lib/libuwspr_hip.so,
    then the host block mirror (gr-uwspr_amd/host) into lib/libuwspr_blocks.so.

    Safe to call from several processes at once (one rank per GPU importing the package at the same moment): the
    check and the build run under a file lock, a build goes to a temporary file that is renamed into place, and
    what decides "current" is the flags + the CONTENTS of the sources (a stamp next to the library) -- not file
    times and not the directory the tree happens to live in, neither of which survives the copy to a GPU box."""
    import fcntl
    if not os.path.isdir(LIBDIR):
        os.makedirs(LIBDIR, exist_ok=True)
    srcs, deps = _sources()
    extra = _EXTRA   # experiments only (separate output file, see LIBPATH)
    flags = HIPFLAGS + extra + ["-shared", "-pthread"]
    hostdir = os.path.join(_HERE, "host")
    hsrcs = [os.path.join(hostdir, f) for f in sorted(os.listdir(hostdir)) if f.endswith(".cc")] \
        if os.path.isdir(hostdir) else []
    hdeps = hsrcs + ([os.path.join(hostdir, f) for f in os.listdir(hostdir) if f.endswith(".h")] if hsrcs else [])
    hflags = ["-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"]

    def atomically(cmd, out):
        tmp = "%s.tmp%d" % (out, os.getpid())
        try:
            if verbose:
                print(" ".join(cmd + ["-o", out]))
            subprocess.run(cmd + ["-o", tmp], check=True)
            os.replace(tmp, out)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    def current(out, want):
        stamp = out + ".cmd"
        return os.path.exists(out) and os.path.exists(stamp) and open(stamp).read() == want

    def stamp(out, want):
        tmp = "%s.cmd.tmp%d" % (out, os.getpid())
        with open(tmp, "w") as f:
            f.write(want)
        os.replace(tmp, out + ".cmd")

    cid = _compiler_id()
    want = " ".join(flags + [os.path.basename(q) for q in srcs]) + "\n" + _digest(deps) + "\n" + cid
    hwant = " ".join(hflags + [os.path.basename(q) for q in hsrcs]) + "\n" + _digest(hdeps + deps) + "\n" + cid

    def all_current():
        return current(LIBPATH, want) and (not hsrcs or bool(extra) or current(HOSTLIB, hwant))

    # the common case -- a shipped, current library -- takes no lock and writes nothing (a read-only tree imports)
    if not force and all_current():
        return LIBPATH
    if cid == "hipcc absent" and not force and os.path.exists(LIBPATH):
        return LIBPATH                       # nothing to rebuild with: the loader decides whether the file is usable
    lock = None
    try:
        lock = open(os.path.join(LIBDIR, ".build.lock"), "w")
        fcntl.flock(lock, fcntl.LOCK_EX)     # (released when the file is closed)
    except OSError as e:                     # EROFS / EACCES: build (if it must) without the lock
        import errno
        if e.errno not in (errno.EROFS, errno.EACCES, errno.EPERM):
            raise
        lock = None
    try:
        if force or not current(LIBPATH, want):
            atomically([_hipcc()] + flags + srcs + ["-ldl"], LIBPATH)
            stamp(LIBPATH, want)
        if hsrcs and not extra:
            if force or not current(HOSTLIB, hwant):
                atomically(["g++"] + hflags + ["-I" + hostdir, "-I" + os.path.join(_HERE, "..", "include")] + hsrcs +
                           ["-L" + LIBDIR, "-luwspr_hip", "-Wl,-rpath,$ORIGIN", "-lpthread"], HOSTLIB)
                stamp(HOSTLIB, hwant)
    finally:
        if lock is not None:
            lock.close()
    return LIBPATH


# ---- ABI structures --------------------------------------------------------
class Params(C.Structure):
    _fields_ = [(k, C.c_int32) for k in
                ("fs", "fl", "spb", "maxdrift", "maxfreqs", "halfbandwidth", "cf", "threshold")]


CAND_DTYPE = np.dtype([("freq", "<f4"), ("snr", "<f4"), ("drift", "<f4"), ("sync", "<f4"),
                       ("shift", "<i4"), ("m_type", "<i4"), ("V1", "<f8"), ("V2", "<f8"),
                       ("p1", "<i4"), ("p2", "<i4")])
HYP_DTYPE = np.dtype([("frame", "<i4"), ("m_type", "<i4"), ("f0", "<f4"), ("lag", "<i4"),
                      ("drift", "<f4"), ("p1", "<i4"), ("p2", "<i4"), ("_pad", "<i4"),
                      ("V1", "<f8"), ("V2", "<f8")])
DEMOD_DTYPE = np.dtype([("f1", "<f4"), ("drift1", "<f4"), ("sync1", "<f4"), ("shift1", "<i4"),
                        ("worth_a_try", "<i4"), ("jig_sync", "<f4", (NJIG,)),
                        ("jig_rms", "<f4", (NJIG,)), ("jig_shift", "<i4", (NJIG,)),
                        ("symbols", "u1", (NJIG, NSYM)), ("_pad", "u1", (2,))])
CALL_DTYPE = np.dtype([("frame", "<i4"), ("_p0", "<i4"), ("candidate", CAND_DTYPE),
                       ("f1", "<f4"), ("ifmin", "<i4"), ("ifmax", "<i4"), ("fstep", "<f4"),
                       ("shift1", "<i4"), ("lagmin", "<i4"), ("lagmax", "<i4"),
                       ("lagstep", "<i4"), ("drift1", "<f4"), ("symfac", "<i4"),
                       ("mode", "<i4"), ("_p1", "<i4")])
RESULT_DTYPE = np.dtype([("sync", "<f4"), ("shift1", "<i4"), ("f1", "<f4"),
                         ("symbols", "u1", (NSYM,)), ("_pad", "u1", (2,))])
assert CAND_DTYPE.itemsize == 48 and HYP_DTYPE.itemsize == 48
assert DEMOD_DTYPE.itemsize == 2980 and CALL_DTYPE.itemsize == 104 and RESULT_DTYPE.itemsize == 176


class Info(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("size", C.c_int32), ("m", C.c_int32),
                ("hpbm", C.c_int32), ("n", C.c_int32), ("finpb", C.c_int32),
                ("noiseidx", C.c_int32), ("df", C.c_float), ("min_snr", C.c_float),
                ("band_lo", C.c_int32), ("band_w", C.c_int32), ("cell_hyps", C.c_int32),
                ("off_min", C.c_int32), ("off_max", C.c_int32), ("device", C.c_int32),
                ("device_name", C.c_char * 64)]


DECODE_DTYPE = np.dtype([("frame", "<i8"), ("stream_pos", "<i8"), ("cand", "<i4"), ("npk", "<i4"),
                         ("coarse", CAND_DTYPE), ("f1", "<f4"), ("drift1", "<f4"), ("sync1", "<f4"),
                         ("shift1", "<i4"), ("worth_a_try", "<i4"), ("decoded", "<i4"), ("idt", "<i4"),
                         ("message", "i1", (7,)), ("block", "u1"), ("channel", "<i2"), ("pass", "u1"), ("osd", "u1")])
assert DECODE_DTYPE.itemsize == 112 and DECODE_DTYPE.fields["channel"][1] == 108 and DECODE_DTYPE.fields["pass"][1] == 110
assert DECODE_DTYPE.fields["osd"][1] == 111 and DECODE_DTYPE.fields["block"][1] == 107
SUB_ITEM_DTYPE = np.dtype([("frame", "<i4"), ("shift", "<i4"), ("f_hz", "<f4"), ("drift_hz", "<f4"),
                           ("symbols", "u1", (NSYM,)), ("_pad", "u1", (2,))])
SUB_RESULT_DTYPE = np.dtype([("f_hz", "<f4"), ("shift", "<i4"), ("metric", "<f4"), ("removed", "<f4")])
assert SUB_ITEM_DTYPE.itemsize == 180 and SUB_RESULT_DTYPE.itemsize == 16
OSD_RESULT_DTYPE = np.dtype([("dmin", "<i4"), ("dnext", "<i4"), ("nhard", "<i4"), ("nflip", "u1"), ("message", "i1", (7,))])
assert OSD_RESULT_DTYPE.itemsize == 20
BLOCK_ITEM_DTYPE = np.dtype([("frame", "<i4"), ("shift", "<i4"), ("f_hz", "<f4"), ("drift_hz", "<f4")])
assert BLOCK_ITEM_DTYPE.itemsize == 16
OSD_GAP_DEFAULT = 485   # UWSPR_OSD_GAP_DEFAULT
DEEP_RESULT_DTYPE = np.dtype([("best", "<i4"), ("sbest", "<i4"), ("snext", "<i4"), ("reserved", "<i4")])
assert DEEP_RESULT_DTYPE.itemsize == 16
DEEP_MAX, DEEP_MIN_DEFAULT, DEEP_GAP_DEFAULT = 65536, 4373, 1145   # UWSPR_DEEP_MAX, UWSPR_DEEP_MIN_DEFAULT, UWSPR_DEEP_GAP_DEFAULT
CALL_RESULT_DTYPE = np.dtype([("best", "<i4"), ("call", "<i4"), ("ngrid", "<i4"), ("dbm", "<i4"), ("sbest", "<i4"), ("snext", "<i4"),
                              ("reserved", "<i4", (2,))])
assert CALL_RESULT_DTYPE.itemsize == 32
CALLS_MAX, CALL_NGRID = 64, 32400   # UWSPR_CALLS_MAX, UWSPR_CALL_NGRID
P19 = (0, 3, 7, 10, 13, 17, 20, 23, 27, 30, 33, 37, 40, 43, 47, 50, 53, 57, 60)   # the type-1 powers in dBm (UWSPR_CALL_NPOW of them)
CALL_MIN_DEFAULT, CALL_GAP_DEFAULT = 5370, 725   # UWSPR_CALL_MIN_DEFAULT, UWSPR_CALL_GAP_DEFAULT
TRACK_TRAJ_DTYPE = np.dtype([("v", "<f8"), ("d", "<f8"), ("tc", "<f8")])
TRACK_RESULT_DTYPE = np.dtype([("best", "<i4"), ("t_best", "<f4"), ("t_ref", "<f4"), ("f_hz", "<f4")])
TRACK_RECORD_DTYPE = np.dtype([("frame", "<i8"), ("cand", "<i4"), ("channel", "<i2"), ("pass", "u1"), ("_pad", "u1"), ("result", TRACK_RESULT_DTYPE)])
assert TRACK_TRAJ_DTYPE.itemsize == 24 and TRACK_RESULT_DTYPE.itemsize == 16 and TRACK_RECORD_DTYPE.itemsize == 32
TRACK_MAX, TRACK_QF_MAX = 4096, 16
FOLLOW_RESULT_DTYPE = np.dtype([("best", "<i4"), ("s_best", "<f4"), ("s_ref", "<f4"), ("f_hz", "<f4")])
FOLLOW_RECORD_DTYPE = np.dtype([("frame", "<i8"), ("cand", "<i4"), ("channel", "<i2"), ("pass", "u1"), ("_pad", "u1"), ("result", FOLLOW_RESULT_DTYPE)])
assert FOLLOW_RESULT_DTYPE.itemsize == 16 and FOLLOW_RECORD_DTYPE.itemsize == 32
FOLLOW_QF_MAX, FOLLOW_NL_MAX = 16, 4   # UWSPR_FOLLOW_QF_MAX, UWSPR_FOLLOW_NL_MAX
FOLLOW_Q, FOLLOW_LSTEP = 375.0 / 2048.0, 32   # K16's frequency step in Hz and lag step in samples
PIPE_MAX_CHANNELS = 64


class TxSignal(C.Structure):
    _fields_ = [("symbols", C.c_uint8 * NSYM), ("_pad", C.c_uint8 * 2), ("channel", C.c_int32), ("start", C.c_int64),
                ("f0_hz", C.c_double), ("drift_hz", C.c_double), ("phase0", C.c_double), ("gain", C.c_float),
                ("_pad2", C.c_int32)]


class TxChannel(C.Structure):
    _fields_ = [("sigma", C.c_double), ("seed", C.c_uint64), ("background", C.c_void_p), ("background_len", C.c_int64),
                ("background_format", C.c_int32), ("background_gain", C.c_float)]




class TxMotion(C.Structure):
    _fields_ = [("v1", C.c_double), ("v2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("t_first", C.c_double),
                ("model", C.c_int32), ("flags", C.c_int32)]


class TxFade(C.Structure):
    _fields_ = [("spread_hz", C.c_double), ("shift_hz", C.c_double), ("k_factor", C.c_double), ("seed", C.c_uint64),
                ("paths", C.c_int32), ("_pad", C.c_int32)]


class TxImpulse(C.Structure):
    _fields_ = [("rate", C.c_double), ("sigma", C.c_double), ("seed", C.c_uint64), ("length", C.c_int32), ("_pad", C.c_int32)]


assert C.sizeof(TxSignal) == 208 and C.sizeof(TxChannel) == 40 and C.sizeof(TxMotion) == 48
assert C.sizeof(TxFade) == 40 and C.sizeof(TxImpulse) == 32
TX_FADE_MAX_PATHS = 32
TX_STATIC, TX_DOPPLER, TX_DELAY = 0, 1, 2
TX_ABSOLUTE, TX_SPREADING = 1, 2


class PipeOpts(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("hop", "batch_frames", "max_per_frame", "lanes", "host_threads", "eager",
                                         "sched_form", "spare_after_us")]


class PipeStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("frames", "batches", "candidates", "decoded", "resumed", "fano_calls",
                                         "fano_timeouts")] + \
               [(k, C.c_double) for k in ("gpu_wait_s", "fano_s", "resume_s")]


K_NAMES = ("spectrogram", "spectrum", "coarse", "tonecorr", "fold", "sched")


class Prof(C.Structure):
    _fields_ = [("ms", C.c_double * 6), ("launches", C.c_int64 * 6), ("units", C.c_int64 * 6)]


# ---- the signatures: name -> (restype, argtypes).  A new C entry point is declared here, in one line, and nowhere else.
_vp, _ip, _ll, _u32, _sz, _str, _P = C.c_void_p, C.c_int, C.c_longlong, C.c_uint32, C.c_size_t, C.c_char_p, C.POINTER
_vp2, _vp3, _vp4 = [_vp] * 2, [_vp] * 3, [_vp] * 4
SIGNATURES = {
    # every symbol include/uwspr_hip.h declares
    "uwspr_ctx_create": (_ip, [_P(Params), _ip, _P(_vp)]),
    "uwspr_ctx_destroy": (None, [_vp]),
    "uwspr_last_error": (_str, [_vp]),
    "uwspr_status_string": (_str, [_ip]),
    "uwspr_get_info": (_ip, [_vp, _P(Info)]),
    "uwspr_set_stream": (_ip, _vp2),
    "uwspr_synchronize": (_ip, [_vp]),
    "uwspr_frontend_batch": (_ip, [_vp, _vp, _ip, _ip, _ip, _vp]),
    "uwspr_frontend_design": (_ip, [_ip, _ip, _vp, _ip, _vp]),
    "uwspr_frontend_design_at": (_ip, [_ip, _ip, _ip, _ip, _vp, _ip, _vp]),
    "uwspr_frontend_rotator": (_ip, [_vp]),
    "uwspr_resample_design": (_ip, [_ip, _vp, _ip] + _vp4),
    "uwspr_resample_batch": (_ip, [_vp, _vp, _ll, _ip, _ip, _ip, _ip, _vp, _ll]),
    "uwspr_blank_batch": (_ip, [_vp, _vp, _ll, _ip, _ip, _ip, _ip, _ip] + _vp3),
    "uwspr_stream_blank_stats": (_ip, _vp3 + [_ip]),
    "uwspr_pipe_blank_stats": (_ip, _vp3 + [_ip]),
    "uwspr_stream_open": (_ip, [_vp, _ip, _ip]),
    "uwspr_stream_push": (_ip, [_vp, _vp, _ip, _ip, _P(_ip)]),
    "uwspr_stream_push_audio": (_ip, [_vp, _vp, _ip, _ip, _ip, _P(_ip)]),
    "uwspr_stream_take": (_ip, [_vp, _ip, _vp, _P(_vp), _P(_ll)]),
    "uwspr_stream_reset": (_ip, [_vp, _ll]),
    "uwspr_set_frame_stride": (_ip, [_vp, _ip]),
    "uwspr_stream_wait_uploads": (_ip, [_vp]),
    "uwspr_stream_take_view": (_ip, [_vp, _ip, _P(_vp), _P(_ip), _P(_ll)]),
    "uwspr_device_alloc": (_ip, [_sz, _P(_vp)]),
    "uwspr_device_free": (None, [_vp]),
    "uwspr_host_alloc": (_ip, [_sz, _P(_vp)]),
    "uwspr_host_free": (None, [_vp]),
    "uwspr_fdr_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _vp]),
    "uwspr_fdr_read_spectrum": (_ip, [_vp, _ip] + _vp4 + [_vp]),
    "uwspr_fdr_keep_syncgrid": (_ip, [_vp, _ip]),
    "uwspr_fdr_read_syncgrid": (_ip, [_vp, _ip, _vp]),
    "uwspr_sync_sweep": (_ip, [_vp, _vp, _ip, _vp, _ip, _ip, _vp, _vp]),
    "uwspr_sync_grid": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp, _ip, _vp, _ip] + _vp3),
    "uwspr_sync_and_demodulate_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp]),
    "uwspr_demod_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _vp, _ip, _ip, _vp]),
    "uwspr_pipeline_batch": (_ip, [_vp, _vp, _ip, _ip, _ip] + _vp3),
    "uwspr_set_tries": (_ip, [_vp, _ip]),
    "uwspr_set_option": (_ip, [_vp, _str, _ip]),
    "uwspr_get_option": (_ip, [_vp, _str, _vp]),
    "uwspr_demod_resume": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp]),
    "uwspr_pack_slabs": (_ip, [_vp, _ip, _ip, _vp, _ip]),
    "uwspr_pipeline_slabs": (_ip, [_vp, _ip, _vp]),
    "uwspr_prof_enable": (_ip, [_vp, _ip]),
    "uwspr_prof_read": (_ip, [_vp, _P(Prof)]),
    "uwspr_prof_intervals": (_ip, [_vp, _ip] + _vp3 + [_ip, _P(_ip)]),
    "uwspr_deinterleave": (None, [_vp]),
    "uwspr_fano_decode": (_ip, [_vp, _vp, _P(_u32), _P(_u32), _P(_u32), _ip, _u32]),
    "uwspr_fano_encode": (_ip, [_vp, _vp, _u32]),
    "uwspr_decode_candidate": (_ip, [_vp, _vp, _P(C.c_int32)]),
    "uwspr_decode_batch": (_ip, [_vp, _ip, _ip] + _vp3),
    "uwspr_host_threads": (_ip, []),
    "uwspr_host_set_ranks": (_ip, [_ip]),
    "uwspr_unpack_message": (_ip, [_vp, _str, _sz]),
    "uwspr_c2_read": (_ip, [_str, _vp, _P(C.c_double), _P(C.c_int32)]),
    "uwspr_wspr_pack": (_ip, [_str, _vp]),
    "uwspr_nhash": (_u32, [_str, _sz, _u32]),
    "uwspr_wspr_symbols": (_ip, _vp2),
    "uwspr_c2_write": (_ip, [_str, _vp, _ip, C.c_double, C.c_int32]),
    "uwspr_tx_baseband": (_ip, _vp2 + [_ip, _ip, _ll, _ip, _vp, _ip]),
    "uwspr_tx_baseband_moving": (_ip, _vp3 + [_ip, _ip, _ll, _ip, _vp, _ip]),
    "uwspr_tx_baseband_at": (_ip, _vp4 + [_ip, _ip, _ll, _ip, _vp, _ip]),
    "uwspr_tx_baseband_medium": (_ip, _vp4 + [_vp, _ip, _ip, _ll, _ip, _vp, _ip]),
    "uwspr_tx_render": (_ip, _vp2 + [_ip, _vp, _ip, _ll, _ll, _ip, _vp, _ip]),
    "uwspr_tx_render_moving": (_ip, _vp3 + [_ip, _vp, _ip, _ll, _ll, _ip, _vp, _ip]),
    "uwspr_tx_render_at": (_ip, _vp4 + [_ip, _vp, _ip, _ll, _ll, _ip, _vp, _ip]),
    "uwspr_tx_render_medium": (_ip, _vp4 + [_vp, _ip, _vp, _vp, _ip, _ll, _ll, _ip, _vp, _ip]),
    "uwspr_tx_design_at": (_ip, [_ip, _ip, _vp, _vp]),
    "uwspr_tx_fade_design": (_ip, _vp4),
    "uwspr_subtract_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _ip, _vp, _vp]),
    "uwspr_osd_batch": (_ip, [_vp, _vp, _ip, _ip, _ip, _vp]),
    "uwspr_blockdemod_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp]),
    "uwspr_deep_set_list": (_ip, [_vp, _vp, _ip]),
    "uwspr_deep_batch": (_ip, [_vp, _vp, _ip, _ip, _vp]),
    "uwspr_calls_set": (_ip, [_vp, _vp, _ip, _vp, _u32]),
    "uwspr_calls_batch": (_ip, [_vp, _vp, _ip, _ip, _vp]),
    "uwspr_call_message": (_ip, [_str, _ip, _ip, _vp]),
    "uwspr_track_design": (_ip, [_vp, _ip, _ip, C.c_double, _vp, _vp]),
    "uwspr_track_from_slm": (_ip, [C.c_double] * 5 + [_vp]),
    "uwspr_track_set": (_ip, [_vp, _vp, _ip, _ip, _ip]),
    "uwspr_track_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp, _vp]),
    "uwspr_follow_set": (_ip, [_vp, _vp, _ip, _ip, _ip, _ip]),
    "uwspr_follow_batch": (_ip, [_vp, _vp, _ip, _ip, _vp, _ip, _vp, _vp, _vp]),
    "uwspr_dist_unique_id": (_ip, [_vp]),
    "uwspr_dist_init": (_ip, [_vp, _ip, _ip, _vp]),
    "uwspr_dist_gather": (_ip, [_vp, _vp, _sz, _vp, _ip, _ip]),
    "uwspr_dist_finalize": (_ip, [_vp]),
    "uwspr_pipe_open": (_ip, [_P(Params), _ip, _P(PipeOpts), _P(_vp)]),
    "uwspr_pipe_close": (None, [_vp]),
    "uwspr_pipe_last_error": (_str, [_vp]),
    "uwspr_pipe_acquire": (_ip, [_vp, _ip, _P(_vp)]),
    "uwspr_pipe_commit": (_ip, [_vp, _ip]),
    "uwspr_pipe_push": (_ip, [_vp, _vp, _ip]),
    "uwspr_pipe_push_audio": (_ip, [_vp, _vp, _ip, _ip]),
    "uwspr_pipe_push_audio_channels": (_ip, [_vp, _vp, _ip, _ip, _ip]),
    "uwspr_pipe_submit_device": (_ip, [_vp, _vp, _ip, _ip]),
    "uwspr_pipe_flush": (_ip, [_vp]),
    "uwspr_pipe_collect": (_ip, [_vp, _vp, _ip, _ip]),
    "uwspr_pipe_get_stats": (_ip, [_vp, _P(PipeStats)]),
    "uwspr_pipe_inject_failure": (_ip, [_vp, _ll, _ip]),
    "uwspr_pipe_set_option": (_ip, [_vp, _str, _ip]),
    "uwspr_pipe_set_carriers": (_ip, [_vp, _vp, _ip]),
    "uwspr_pipe_set_list": (_ip, [_vp, _vp, _ip]),
    "uwspr_pipe_set_calls": (_ip, [_vp, _vp, _ip, _vp, _u32]),
    "uwspr_pipe_set_tracks": (_ip, [_vp, _vp, _ip, _ip, _ip]),
    "uwspr_pipe_collect_tracks": (_ip, [_vp, _vp, _ip]),
    "uwspr_pipe_set_follow": (_ip, [_vp, _vp, _ip, _ip, _ip, _ip]),
    "uwspr_pipe_collect_follows": (_ip, [_vp, _vp, _ip]),
    # diagnostics, outside the ABI header (defined extern "C" under csrc/)
    "uwspr_debug_fdr_from_ps": (_ip, [_vp, _vp, _ip, _ip, _vp, _vp]),
    "uwspr_debug_snr_db": (_ip, _vp3 + [_ll]),
    "uwspr_debug_launch_forms": (_ip, [_vp, _vp, _ip]),
    "uwspr_debug_frontend_launch": (_ip, [_vp, _vp, _ip, _ip, _ll, _ip, _vp, _ip, _ll, _ll]),
    "uwspr_debug_frontend_carrier_launch": (_ip, [_vp, _vp, _ip, _ip, _ll, _ip, _ip, _vp, _vp, _ip, _ll, _ll]),
    "uwspr_debug_resample_launch": (_ip, [_vp, _vp, _ip, _ll, _ll, _ip, _ip, _vp, _ll, _ll]),
    "uwspr_debug_blank_launch": (_ip, [_vp, _vp, _ip, _ll, _ll, _ip, _vp, _ll, _ll, _ll, _ll, _ip, _ip, _vp, _ll, _ll, _vp]),
    "uwspr_debug_tx_taps": (_ip, _vp2),
    "uwspr_debug_tx_carrier_counts": (_ip, [_vp]),
    "uwspr_debug_tx_medium_counts": (_ip, [_vp]),
    "uwspr_debug_frontend_carrier_counts": (_ip, [_vp]),
    "uwspr_debug_resample_counts": (_ip, [_vp]),
    "uwspr_debug_blank_counts": (_ip, [_vp]),
    "uwspr_debug_track_time": (_ip, [_vp, _ip, _vp]),
    "uwspr_debug_follow_time": (_ip, [_vp, _ip, _vp]),
}
ABI_SYMBOLS = [k for k in SIGNATURES if not k.startswith("uwspr_debug_")]

_lib = None


def lib():
    """Load (building first if needed) the shared library.  Fails loudly."""
    global _lib
    if _lib is not None:
        return _lib
    # always through build(): the command stamp + mtime check is cheap and a stale or foreign
    # library is never loaded silently.  Where the sources cannot be compiled (no hipcc on a
    # deployment box) an existing library is used as it is.
    try:
        build()
    except (UwsprError, subprocess.CalledProcessError, OSError):
        if not os.path.exists(LIBPATH):
            raise
    # One HIP/HSA runtime per process: PyTorch bundles its own libamdhip64.so.7 /
    # libhsa-runtime64 and this library is linked against /opt/rocm's (same SONAME).
    # Whichever is loaded first serves both; two live copies leave the second one
    # without a device.  Load torch's first whenever torch is going to be used.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIBPATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(L, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = L
    return L
