"""gr-uwspr_amd -- MI355X (gfx950) implementation of gr-uwspr's coarse (FDR) and
fine (sync_and_demodulate) search path behind the C ABI in include/uwspr_hip.h.

    csrc/     hand-written HIP kernels K0..K16 + the C ABI + the host tail
    host/     C++ mirror of the gr::uwspr block API on top of the C ABI
    native.py build (hipcc, gfx950) + ctypes binding
    context.py thin Python handle used by tests/ and bench.py
    synth.py  seeded synthetic frame generator (test/bench input only)
    dist.py   frame sharding + candidate gather across ranks (RCCL/gloo)

The directory name has a hyphen; import it as `gr_uwspr_amd` (root shim).
"""
from . import native  # noqa: F401
from .native import UwsprError, build  # noqa: F401
from .context import (Context, FrameView, Pipe, host_threads, host_set_ranks, deinterleave, fano_decode, fano_encode, decode_candidate, decode_batch,  # noqa: F401
                      unpack_message, c2_read, frontend_design, FRONTEND_GRC, FRONTEND_COMPACT, host_alloc, host_free,
                      read_wav, decode_wav, wspr_pack, nhash, wspr_symbols, write_c2, tx_signals, tx_sigma, encode_wav,
                      tx_motions, slm_trajectories, slm_drift, sub_items, block_items, resample_design, resample_launch_counts, frontend_rotator, frontend_carrier_launch_counts,
                      supported_rate, blank_launch_counts, BLANK_BLOCK, tx_taps, tx_design,
                      tx_carriers, tx_carrier_launch_counts, tx_fades, tx_impulses, tx_fade_design, tx_medium_launch_counts, call_message, grids_bitmap, grid_ngrid, powers_mask,
                      track_trajs, track_grid, track_from_slm, track_doppler, track_design, track_motion)
from . import synth  # noqa: F401
from .sweep import sweep_grid, sweep_grid_uniform  # noqa: F401
