"""ctypes binding of the batch interface (Part 2 of include/ldpc_amd.h)."""
import ctypes as ct
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# LDPC_AMD_LIB selects another build of the library (same-box A/B runs, tools/ab.sh); the default is the in-tree product
LIB_PATH = os.environ.get("LDPC_AMD_LIB") or os.path.join(PKG, "libldpc.so")

AWGN, BSC, BEC = 1, 2, 3
CHANNELS = {"AWGN": AWGN, "BSC": BSC, "BEC": BEC}


class decoder_param(ct.Structure):
    _fields_ = [("earlyTerm", ct.c_bool), ("iterations", ct.c_uint32), ("type", ct.c_char_p)]


class channel_param(ct.Structure):
    _fields_ = [("seed", ct.c_uint64), ("xRange", ct.c_double * 3), ("type", ct.c_char_p)]


class simulation_param(ct.Structure):
    _fields_ = [("threads", ct.c_uint32), ("maxFrames", ct.c_uint64), ("fec", ct.c_uint64),
                ("resultFile", ct.c_char_p)]


class sim_results_t(ct.Structure):
    _fields_ = [("fer", ct.POINTER(ct.c_double)), ("ber", ct.POINTER(ct.c_double)),
                ("avg_iter", ct.POINTER(ct.c_double)), ("time", ct.POINTER(ct.c_double)),
                ("fec", ct.POINTER(ct.c_uint64)), ("frames", ct.POINTER(ct.c_uint64))]


class ldpc_hip_out(ct.Structure):
    _fields_ = [("iters", ct.c_void_p), ("bit_errors", ct.c_void_p), ("hard", ct.c_void_p),
                ("llr_out", ct.c_void_p), ("llr_in", ct.c_void_p), ("codeword", ct.c_void_p)]


class ldpc_hip_channel(ct.Structure):
    _fields_ = [("channel", ct.c_int), ("x", ct.c_double), ("seed", ct.c_uint64), ("first_frame", ct.c_uint64),
                ("bits_per_symbol", ct.c_int), ("llr_type", ct.c_int), ("q_bits", ct.c_int), ("step", ct.c_double)]


class ldpc_hip_syndrome_decode(ct.Structure):
    _fields_ = [("iterations", ct.c_uint32), ("early_term", ct.c_int), ("q_bits", ct.c_int), ("step", ct.c_double),
                ("scale", ct.c_double), ("offset", ct.c_double), ("flags", ct.c_int)]


class ldpc_hip_syndrome_decode_layered(ct.Structure):
    _fields_ = [("iterations", ct.c_uint32), ("early_term", ct.c_int), ("msg_bits", ct.c_int), ("app_bits", ct.c_int),
                ("step", ct.c_double), ("scale", ct.c_double), ("offset", ct.c_double), ("flags", ct.c_int)]


class ldpc_hip_bit_flip(ct.Structure):
    _fields_ = [("iterations", ct.c_uint32), ("q_bits", ct.c_int), ("step", ct.c_double), ("check_weight", ct.c_uint32),
                ("margin", ct.c_uint32), ("flip_threshold", ct.c_uint32), ("seed", ct.c_uint64), ("first_frame", ct.c_uint64),
                ("flags", ct.c_int)]


class ldpc_hip_relay_decode(ct.Structure):
    _fields_ = [("legs", ct.c_uint32), ("first_iterations", ct.c_uint32), ("leg_iterations", ct.c_uint32), ("stop_after", ct.c_uint32),
                ("q_bits", ct.c_int), ("step", ct.c_double), ("scale", ct.c_double), ("offset", ct.c_double), ("form", ct.c_int),
                ("flags", ct.c_int)]


_lib = None


def load_library(path=LIB_PATH):
    """Load libldpc.so; raises if it has not been built (python -m libldpc_amd.build)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"{path} is missing: build the HIP extension first (python -m libldpc_amd.build); "
                      "there is no CPU fallback")
    L = ct.CDLL(path)
    vp, u64, i32 = ct.c_void_p, ct.c_uint64, ct.c_int
    L.ldpc_hip_device_count.restype = i32
    L.ldpc_hip_last_error.restype = ct.c_char_p
    L.ldpc_hip_create.restype = vp
    L.ldpc_hip_create.argtypes = [ct.c_char_p, ct.c_char_p, i32]
    L.ldpc_hip_destroy.argtypes = [vp]
    L.ldpc_hip_code_info.argtypes = [vp, ct.POINTER(ct.c_int64)]
    L.ldpc_hip_set_bec_compat.argtypes = [vp, i32]
    L.ldpc_hip_set_fast_mode.argtypes = [vp, i32]
    L.ldpc_hip_set_noise.restype = i32
    L.ldpc_hip_set_noise.argtypes = [vp, i32]
    L.ldpc_hip_set_min_sum_correction.restype = i32
    L.ldpc_hip_set_min_sum_correction.argtypes = [vp, ct.c_double, ct.c_double]
    L.ldpc_hip_set_min_sum_schedule.restype = i32
    L.ldpc_hip_set_min_sum_schedule.argtypes = [vp, i32]
    L.ldpc_hip_min_sum_schedule.restype = i32
    L.ldpc_hip_min_sum_schedule.argtypes = [vp]
    L.ldpc_hip_layered_min_sum_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_layered_min_sum_lds_bytes.argtypes = [vp]
    L.ldpc_hip_set_min_sum_quantization.restype = i32
    L.ldpc_hip_set_min_sum_quantization.argtypes = [vp, i32, ct.c_double]
    L.ldpc_hip_min_sum_quantization.restype = i32
    L.ldpc_hip_min_sum_quantization.argtypes = [vp, ct.POINTER(i32), ct.POINTER(ct.c_double)]
    L.ldpc_hip_quantized_min_sum_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_quantized_min_sum_lds_bytes.argtypes = [vp]
    L.ldpc_hip_set_min_sum_ternary.restype = i32
    L.ldpc_hip_set_min_sum_ternary.argtypes = [vp, i32]
    L.ldpc_hip_min_sum_ternary.restype = i32
    L.ldpc_hip_min_sum_ternary.argtypes = [vp]
    L.ldpc_hip_ternary_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_ternary_lds_bytes.argtypes = [vp]
    L.ldpc_hip_set_min_sum_layered_fixed.restype = i32
    L.ldpc_hip_set_min_sum_layered_fixed.argtypes = [vp, i32, i32, ct.c_double]
    L.ldpc_hip_min_sum_layered_fixed.restype = i32
    L.ldpc_hip_min_sum_layered_fixed.argtypes = [vp, ct.POINTER(i32), ct.POINTER(i32), ct.POINTER(ct.c_double)]
    L.ldpc_hip_layered_fixed_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_layered_fixed_lds_bytes.argtypes = [vp]
    L.ldpc_hip_philox.restype = i32
    L.ldpc_hip_philox.argtypes = [vp, u64, ct.c_uint32, u64, ct.c_uint32, u64, vp, vp]
    L.ldpc_hip_decode_batch.restype = i32
    L.ldpc_hip_decode_batch.argtypes = [vp, decoder_param, u64, vp, ct.POINTER(ldpc_hip_out), vp]
    L.ldpc_hip_decode_batch_typed.restype = i32
    L.ldpc_hip_decode_batch_typed.argtypes = [vp, decoder_param, u64, vp, i32, ct.POINTER(ldpc_hip_out), vp, vp]
    L.ldpc_hip_layered_fixed_direct_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_layered_fixed_direct_lds_bytes.argtypes = [vp]
    L.ldpc_hip_encode_batch.restype = i32
    L.ldpc_hip_encode_batch.argtypes = [vp, u64, vp, i32, vp, vp, vp]
    L.ldpc_hip_syndrome_batch.restype = i32
    L.ldpc_hip_syndrome_batch.argtypes = [vp, u64, vp, i32, vp, vp, vp, vp]
    L.ldpc_hip_bit_errors_batch.restype = i32
    L.ldpc_hip_bit_errors_batch.argtypes = [vp, u64, vp, i32, vp, i32, vp, vp]
    L.ldpc_hip_channel_batch.restype = i32
    L.ldpc_hip_channel_batch.argtypes = [vp, ct.POINTER(ldpc_hip_channel), u64, vp, i32, vp, vp, vp]
    L.ldpc_hip_erasure_channel_batch.restype = i32
    L.ldpc_hip_erasure_channel_batch.argtypes = [vp, ct.c_double, u64, u64, u64, vp, i32, vp, vp, vp]
    L.ldpc_hip_erasure_decode_batch.restype = i32
    L.ldpc_hip_erasure_decode_batch.argtypes = [vp, ct.c_uint32, i32, u64, vp, vp, i32, vp, vp, vp, vp, vp]
    L.ldpc_hip_erasure_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_erasure_lds_bytes.argtypes = [vp]
    L.ldpc_hip_erasure_solve_batch.restype = i32
    L.ldpc_hip_erasure_solve_batch.argtypes = [vp, ct.c_uint32, u64, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ldpc_hip_erasure_solve_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_erasure_solve_lds_bytes.argtypes = [vp, ct.c_uint32]
    L.ldpc_hip_osd_batch.restype = i32
    L.ldpc_hip_osd_batch.argtypes = [vp, ct.c_uint32, u64, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ldpc_hip_osd_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_osd_lds_bytes.argtypes = [vp]
    L.ldpc_hip_osd_syndrome_batch.restype = i32
    L.ldpc_hip_osd_syndrome_batch.argtypes = [vp, ct.c_uint32, ct.c_uint32, u64, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.ldpc_hip_osd_syndrome_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_osd_syndrome_lds_bytes.argtypes = [vp]
    L.ldpc_hip_syndrome_decode_batch.restype = i32
    L.ldpc_hip_syndrome_decode_batch.argtypes = [vp, ct.POINTER(ldpc_hip_syndrome_decode), u64, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    L.ldpc_hip_syndrome_decode_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_syndrome_decode_lds_bytes.argtypes = [vp]
    L.ldpc_hip_syndrome_decode_layered_batch.restype = i32
    L.ldpc_hip_syndrome_decode_layered_batch.argtypes = [vp, ct.POINTER(ldpc_hip_syndrome_decode_layered), u64, vp, i32, vp, i32, vp, vp, vp,
                                                         vp, vp]
    L.ldpc_hip_syndrome_decode_layered_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_syndrome_decode_layered_lds_bytes.argtypes = [vp]
    L.ldpc_hip_bit_flip_batch.restype = i32
    L.ldpc_hip_bit_flip_batch.argtypes = [vp, ct.POINTER(ldpc_hip_bit_flip), u64, vp, i32, vp, i32, vp, vp, vp, vp]
    L.ldpc_hip_bit_flip_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_bit_flip_lds_bytes.argtypes = [vp]
    L.ldpc_hip_relay_decode_batch.restype = i32
    L.ldpc_hip_relay_decode_batch.argtypes = [vp, ct.POINTER(ldpc_hip_relay_decode), u64, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ldpc_hip_relay_decode_lds_bytes.restype = ct.c_int64
    L.ldpc_hip_relay_decode_lds_bytes.argtypes = [vp, i32]
    L.ldpc_hip_stream_begin.restype = i32
    L.ldpc_hip_stream_begin.argtypes = [vp, i32, u64, ct.c_double]
    L.ldpc_hip_stream_skip.restype = i32
    L.ldpc_hip_stream_skip.argtypes = [vp, u64, vp]
    L.ldpc_hip_stream_decode.restype = i32
    L.ldpc_hip_stream_decode.argtypes = [vp, decoder_param, u64, ct.POINTER(ldpc_hip_out), vp]
    L.ldpc_hip_stream_frame.restype = u64
    L.ldpc_hip_stream_frame.argtypes = [vp]
    L.ldpc_hip_stream_raw_draws.restype = u64
    L.ldpc_hip_stream_raw_draws.argtypes = [vp]
    L.ldpc_hip_synchronize.restype = i32
    L.ldpc_hip_synchronize.argtypes = [vp, vp]
    L.ldpc_hip_batch_counters.restype = i32
    L.ldpc_hip_batch_counters.argtypes = [vp, vp, vp, u64, ct.c_uint32, i32, vp, vp]
    L.ldpc_hip_selftest_division.restype = i32
    L.ldpc_hip_selftest_division.argtypes = [vp, u64, u64, vp]
    L.ldpc_hip_mt64.restype = i32
    L.ldpc_hip_mt64.argtypes = [vp, u64, u64, u64, vp, vp]
    L.ldpc_hip_set_profiling.argtypes = [vp, i32]
    L.ldpc_hip_last_ms.restype = ct.c_float
    L.ldpc_hip_last_ms.argtypes = [vp, i32]
    L.ldpc_hip_comm_unique_id.restype = i32
    L.ldpc_hip_comm_unique_id.argtypes = [vp]
    L.ldpc_hip_comm_create.restype = vp
    L.ldpc_hip_comm_create.argtypes = [i32, i32, i32, vp]
    L.ldpc_hip_comm_create_shm.restype = vp
    L.ldpc_hip_comm_create_shm.argtypes = [i32, i32, ct.c_char_p]
    L.ldpc_hip_comm_create_echo.restype = vp
    L.ldpc_hip_comm_create_echo.argtypes = [i32, i32]
    L.ldpc_hip_comm_destroy.argtypes = [vp]
    L.ldpc_hip_comm_allgather.restype = i32
    L.ldpc_hip_comm_allgather.argtypes = [vp, vp, vp, u64]
    L.ldpc_hip_fused_plan_info.restype = None
    L.ldpc_hip_fused_plan_info.argtypes = [vp, vp]
    L.ldpc_hip_fused_program.restype = i32
    L.ldpc_hip_fused_program.argtypes = [vp]
    L.ldpc_hip_decode_stages.restype = i32
    L.ldpc_hip_decode_stages.argtypes = [vp, decoder_param, vp]
    L.ldpc_hip_decoder_choice.restype = i32
    L.ldpc_hip_decoder_choice.argtypes = [vp, decoder_param]
    L.ldpc_hip_selftest_sim_fold.restype = i32
    L.ldpc_hip_selftest_sim_fold.argtypes = [vp, vp, u64, vp, u64, i32, u64, u64, vp]
    L.ldpc_hip_selftest_layer_plan.restype = i32
    L.ldpc_hip_selftest_layer_plan.argtypes = [vp, vp]
    L.ldpc_hip_selftest_place.restype = i32
    L.ldpc_hip_selftest_place.argtypes = [vp, u64, u64, u64, u64, u64, u64, u64, vp]
    L.ldpc_hip_comm_stats.restype = None
    L.ldpc_hip_comm_stats.argtypes = [vp, vp, i32]
    L.ldpc_hip_comm_describe.restype = ct.c_char_p
    L.ldpc_hip_comm_describe.argtypes = [vp]
    L.ldpc_hip_shard_capacity.restype = u64
    L.ldpc_hip_shard_capacity.argtypes = [vp, u64, i32]
    L.ldpc_hip_stream_decode_sharded.restype = i32
    L.ldpc_hip_stream_decode_sharded.argtypes = [vp, vp, decoder_param, u64, ct.POINTER(ldpc_hip_out), vp, vp]
    L.ldpc_hip_simulate_sharded.restype = i32
    L.ldpc_hip_simulate_sharded.argtypes = [vp, vp, decoder_param, channel_param, simulation_param, ct.POINTER(sim_results_t),
                                            vp, ct.POINTER(ct.c_bool), i32]
    L.ldpc_hip_selftest_math.restype = i32
    L.ldpc_hip_selftest_math.argtypes = [vp, i32, u64, vp, vp, vp]
    L.ldpc_hip_selftest_chunk_table.restype = u64
    L.ldpc_hip_selftest_chunk_table.argtypes = [u64, u64, u64, u64]
    L.ldpc_hip_selftest_shard_table.restype = u64
    L.ldpc_hip_selftest_shard_table.argtypes = [i32, i32, ct.c_uint32, u64, vp]
    L.ldpc_hip_jump_tasks.restype = u64
    L.ldpc_hip_jump_tasks.argtypes = [vp]
    L.ldpc_hip_simulate.restype = i32
    L.ldpc_hip_simulate.argtypes = [vp, decoder_param, channel_param, simulation_param, ct.POINTER(sim_results_t),
                                    vp, ct.POINTER(ct.c_bool), i32]
    if path == LIB_PATH:
        _lib = L
    return L


def _ptr(buf):
    """Address of a numpy array or of a torch tensor (host or device)."""
    if buf is None:
        return None
    if isinstance(buf, np.ndarray):
        assert buf.flags["C_CONTIGUOUS"]
        return buf.ctypes.data
    if hasattr(buf, "data_ptr"):
        assert buf.is_contiguous()
        return buf.data_ptr()
    raise TypeError(f"unsupported buffer type {type(buf)}")


def _dec(early_term, iterations, decoding):
    return decoder_param(bool(early_term), int(iterations), decoding.encode())


def sim_fold(iters, bit_errors, ends, world=1, min_fec=50, max_frames=10**10, lib=LIB_PATH):
    """The simulation loop's counters over given per-frame results, cut into ranges ending at `ends`, `world` ranges to a
    step (include/ldpc_amd.h, ldpc_hip_selftest_sim_fold; no GPU): (steps walked, the eight output words)."""
    it, be = np.ascontiguousarray(iters, np.uint32), np.ascontiguousarray(bit_errors, np.uint32)
    e = np.ascontiguousarray(ends, np.uint64)
    out = np.zeros(8, np.uint64)
    steps = load_library(lib).ldpc_hip_selftest_sim_fold(_ptr(it), _ptr(be), min(it.size, be.size), _ptr(e), e.size, int(world),
                                                         int(min_fec), int(max_frames), _ptr(out))
    return steps, [int(v) for v in out]


class Comm:
    """The exchange between the ranks of a sharded simulation (include/ldpc_amd.h part 3): RCCL when `unique_id` (128
    bytes from Comm.unique_id() on rank 0) is given, host shared memory when `shm_name` is."""

    def __init__(self, rank, world, device=0, unique_id=None, shm_name=None, echo=False, lib=LIB_PATH):
        self.lib = load_library(lib)
        self.rank, self.world = int(rank), int(world)
        if echo:  # one process standing in for one rank of `world` (cost probes): no transport
            self.handle = self.lib.ldpc_hip_comm_create_echo(self.rank, self.world)
        elif shm_name is not None:
            self.handle = self.lib.ldpc_hip_comm_create_shm(self.rank, self.world, shm_name.encode())
        else:
            buf = (ct.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
            self.handle = self.lib.ldpc_hip_comm_create(self.rank, self.world, int(device), buf)
        if not self.handle:
            raise RuntimeError("communicator: " + self.lib.ldpc_hip_last_error().decode())

    @staticmethod
    def unique_id(lib=LIB_PATH):
        L = load_library(lib)
        buf = (ct.c_uint8 * 128)()
        if L.ldpc_hip_comm_unique_id(buf) != 0:
            raise RuntimeError("ldpc_hip_comm_unique_id: " + L.ldpc_hip_last_error().decode())
        return bytes(buf)

    def all_gather(self, values):
        """values: 1-D uint64 array (at most 32 words) -> [world][len] array"""
        v = np.ascontiguousarray(values, np.uint64)
        out = np.zeros((self.world, v.size), np.uint64)
        if self.lib.ldpc_hip_comm_allgather(self.handle, v.ctypes.data, out.ctypes.data, v.nbytes) != 0:
            raise RuntimeError("ldpc_hip_comm_allgather: " + self.lib.ldpc_hip_last_error().decode())
        return out

    def place(self, nct, pairs_before, frame_pos, cap, piece_pairs, pairs_with_margin, status=0):
        """The placement step of a sharded AWGN step over this communicator (no GPU): (first frame, frames of this rank,
        frames of the step, first pair of the piece, first pair after the step)."""
        out = (ct.c_uint64 * 5)()
        if self.lib.ldpc_hip_selftest_place(self.handle, nct, pairs_before, frame_pos, cap, piece_pairs, pairs_with_margin, status, out) != 0:
            raise RuntimeError("ldpc_hip_selftest_place: " + self.lib.ldpc_hip_last_error().decode())
        return tuple(int(v) for v in out)

    def exchange_stats(self, reset=False):
        """host microseconds inside the all-gathers since the last reset: {"calls", "min", "median", "max"}"""
        out = (ct.c_double * 4)()
        self.lib.ldpc_hip_comm_stats(self.handle, out, int(reset))
        return {"calls": int(out[0]), "min": out[1], "median": out[2], "max": out[3]}

    def describe(self):
        return self.lib.ldpc_hip_comm_describe(self.handle).decode()

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ldpc_hip_comm_destroy(self.handle)
            self.handle = None

    __del__ = close


class HipDecoder:
    """One code on one GPU.  All batch calls take numpy arrays or torch tensors as buffers."""

    OUT_SPEC = {"iters": (np.uint32, False), "bit_errors": (np.uint32, False), "hard": (np.uint8, True),
                "llr_out": (np.float64, True), "llr_in": (np.float64, True), "codeword": (np.uint8, True)}

    def __init__(self, pc_file, gen_file="", device=0, lib=LIB_PATH):
        self.lib = load_library(lib)
        self.ctx = self.lib.ldpc_hip_create(pc_file.encode(), gen_file.encode(), device)
        if not self.ctx:
            raise RuntimeError("ldpc_hip_create: " + self.lib.ldpc_hip_last_error().decode())
        info = (ct.c_int64 * 10)()
        self.lib.ldpc_hip_code_info(self.ctx, info)
        (self.nc, self.mc, self.nnz, self.nct, self.mct, self.kct, self.kc, self.max_degree, lds,
         self.lds_bytes) = list(info)
        self.lds_resident = lds == 1
        self.residency = {0: "memory", 1: "lds", 2: "registers", 3: "registers"}[int(lds)]
        self.register_form = {2: "messages", 3: "totals"}.get(int(lds))  # which register-resident kernel

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ldpc_hip_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: " + self.lib.ldpc_hip_last_error().decode())

    def _outs(self, n, want, out):
        """Build the output struct; `want` names host (numpy) outputs to allocate, `out` passes buffers."""
        bufs = dict(out or {})
        for name in want:
            if name not in bufs:
                dt, per_bit = self.OUT_SPEC[name]
                bufs[name] = np.zeros((n, self.nc) if per_bit else (n,), dt)
        s = ldpc_hip_out(*[_ptr(bufs.get(k)) for k in ("iters", "bit_errors", "hard", "llr_out", "llr_in", "codeword")])
        return s, bufs

    def set_bec_compat(self, on):
        self.lib.ldpc_hip_set_bec_compat(self.ctx, int(on))

    def fused_plan(self):
        """Summary of the plan of the fused form (include/ldpc_amd.h, ldpc_hip_fused_plan_info)."""
        info = (ct.c_int64 * 8)()
        self.lib.ldpc_hip_fused_plan_info(self.ctx, info)
        return dict(zip(("ok", "n_slots", "vnb", "cnl", "small", "calls_stride", "has_shortened", "table_entries"), [int(v) for v in info]))

    def fused_program(self):
        """Index of the compile-time wave program the fused plan matches (include/ldpc_amd.h, ldpc_hip_fused_program), or -1:
        the plan is interpreted.  Touches no GPU."""
        return int(self.lib.ldpc_hip_fused_program(self.ctx))

    STAGES = ("whole", "ratio-first", "ratio-separate", "list-chain", "llr-redo", "handover-first", "handover-resume")

    def decode_stages(self, early_term=True, iterations=50, decoding="BP"):
        """The launches a batch with these parameters takes, in order (include/ldpc_amd.h, ldpc_hip_decode_stages; honours
        set_fast_mode; touches no GPU)."""
        stages = (ct.c_int32 * 3)()
        n = self.lib.ldpc_hip_decode_stages(self.ctx, _dec(early_term, iterations, decoding), stages)
        return [self.STAGES[stages[i]] for i in range(n)]

    DECODERS = ("resident", "fast32", "layered32", "layered16", "layered-min-sum", "quantized-min-sum", "ternary",
                "layered-fixed-min-sum")

    def decoder_choice(self, early_term=True, iterations=50, decoding="BP"):
        """The decoder that runs a batch with these parameters under the switches in force (include/ldpc_amd.h,
        ldpc_hip_decoder_choice; touches no GPU)."""
        return self.DECODERS[self.lib.ldpc_hip_decoder_choice(self.ctx, _dec(early_term, iterations, decoding))]

    def set_fast_mode(self, on):
        """Opt-in NON-PARITY mode: sum-product with binary32 messages (include/ldpc_amd.h)."""
        self.lib.ldpc_hip_set_fast_mode(self.ctx, int(on))

    NOISE_MODES = {"reference": 0, "counter": 1}

    def set_noise(self, mode):
        """Noise of the stream interface from the next stream_begin on: "reference" (the default: the reference's
        mt19937_64 stream, parity) or "counter" (Philox4x32-10 of (seed, frame, bit): NON-PARITY, include/ldpc_amd.h)."""
        m = self.NOISE_MODES.get(mode, mode) if isinstance(mode, str) else int(mode)
        if isinstance(m, str):
            m = -1
        self._check(self.lib.ldpc_hip_set_noise(self.ctx, int(m)), f"ldpc_hip_set_noise({mode!r})")

    def set_min_sum_correction(self, scale=1.0, offset=0.0):
        """Corrected min-sum for every "BP_MS" decode from the next call on: check-node output magnitudes
        max(fl(fl(scale * m) - offset), +0.0), normalized (scale < 1) and offset (offset > 0) min-sum.  NON-PARITY unless
        (1, 0), which switches it off (include/ldpc_amd.h).  0 < scale <= 1, 0 <= offset <= 1e6; touches no GPU."""
        self._check(self.lib.ldpc_hip_set_min_sum_correction(self.ctx, float(scale), float(offset)),
                    f"ldpc_hip_set_min_sum_correction({scale!r}, {offset!r})")

    MS_SCHEDULES = {"flooding": 0, "layered": 1}

    def set_min_sum_schedule(self, schedule):
        """Schedule of every "BP_MS" decode from the next call on: "flooding" (the default, the reference's) or "layered"
        (row-serial, NON-PARITY; include/ldpc_amd.h, ldpc_hip_set_min_sum_schedule).  Combines with set_min_sum_correction and
        both noise modes; raises, leaving the setting as it is, for a code the layered kernel does not take.  Touches no GPU."""
        m = self.MS_SCHEDULES.get(schedule, -1) if isinstance(schedule, str) else int(schedule)
        self._check(self.lib.ldpc_hip_set_min_sum_schedule(self.ctx, int(m)), f"ldpc_hip_set_min_sum_schedule({schedule!r})")

    @property
    def min_sum_schedule(self):
        """The schedule of "BP_MS" decoding in force: "flooding" or "layered"."""
        return ("flooding", "layered")[int(self.lib.ldpc_hip_min_sum_schedule(self.ctx))]

    def layered_min_sum_lds_bytes(self):
        """LDS bytes one frame of layered min-sum takes (-1: the layered plan does not take the code)."""
        return int(self.lib.ldpc_hip_layered_min_sum_lds_bytes(self.ctx))

    def set_min_sum_quantization(self, bits=0, step=1.0):
        """Quantized (fixed-point) min-sum for every "BP_MS" decode from the next call on: messages of `bits` bits (2..8; 0 =
        off, the default) on a saturating integer datapath with LLR step `step` (NON-PARITY; include/ldpc_amd.h,
        ldpc_hip_set_min_sum_quantization).  Combines with set_min_sum_correction and both noise modes, not with the layered
        schedule; raises, leaving the setting as it is, for invalid values or a code the kernel does not take.  Touches no GPU."""
        self._check(self.lib.ldpc_hip_set_min_sum_quantization(self.ctx, int(bits), float(step)),
                    f"ldpc_hip_set_min_sum_quantization({bits!r}, {step!r})")

    @property
    def min_sum_quantization(self):
        """(bits, step) of quantized min-sum in force; bits 0 = off."""
        bits, step = ct.c_int32(0), ct.c_double(0.0)
        self.lib.ldpc_hip_min_sum_quantization(self.ctx, ct.byref(bits), ct.byref(step))
        return int(bits.value), float(step.value)

    def quantized_min_sum_lds_bytes(self):
        """LDS bytes one frame of quantized min-sum takes (-1: the kernel does not take the code)."""
        return int(self.lib.ldpc_hip_quantized_min_sum_lds_bytes(self.ctx))

    def set_min_sum_ternary(self, weight=0):
        """Ternary min-sum (Gallager's Algorithm E, messages in {-1, 0, +1}) for every "BP_MS" decode from the next call on,
        with channel weight `weight` (1..7; 0 = off, the default).  NON-PARITY; include/ldpc_amd.h, ldpc_hip_set_min_sum_ternary.
        Combines with both noise modes, not with the layered schedule or quantization; set_min_sum_correction has no effect
        while it is on.  Raises, leaving the setting as it is, for invalid values or a code the kernel does not take.
        Touches no GPU."""
        self._check(self.lib.ldpc_hip_set_min_sum_ternary(self.ctx, int(weight)), f"ldpc_hip_set_min_sum_ternary({weight!r})")

    @property
    def min_sum_ternary(self):
        """The channel weight of ternary min-sum in force; 0 = off."""
        return int(self.lib.ldpc_hip_min_sum_ternary(self.ctx))

    def ternary_lds_bytes(self):
        """LDS bytes one 32-frame group of ternary min-sum takes (-1: the kernel does not take the code)."""
        return int(self.lib.ldpc_hip_ternary_lds_bytes(self.ctx))

    def set_min_sum_layered_fixed(self, msg_bits=0, app_bits=8, step=1.0):
        """Fixed-point layered min-sum for every "BP_MS" decode from the next call on: the layered schedule with messages of
        `msg_bits` bits (2..8; 0 = off, the default), saturating totals of `app_bits` bits (msg_bits..16) and LLR step `step`
        (NON-PARITY; include/ldpc_amd.h, ldpc_hip_set_min_sum_layered_fixed).  Combines with set_min_sum_correction and both
        noise modes, not with the layered schedule, quantization or ternary min-sum; raises, leaving the setting as it is, for
        invalid values or a code the kernel does not take.  Touches no GPU."""
        self._check(self.lib.ldpc_hip_set_min_sum_layered_fixed(self.ctx, int(msg_bits), int(app_bits), float(step)),
                    f"ldpc_hip_set_min_sum_layered_fixed({msg_bits!r}, {app_bits!r}, {step!r})")

    @property
    def min_sum_layered_fixed(self):
        """(msg_bits, app_bits, step) of fixed-point layered min-sum in force; msg_bits 0 = off."""
        q, p, step = ct.c_int32(0), ct.c_int32(0), ct.c_double(0.0)
        self.lib.ldpc_hip_min_sum_layered_fixed(self.ctx, ct.byref(q), ct.byref(p), ct.byref(step))
        return int(q.value), int(p.value), float(step.value)

    def layered_fixed_lds_bytes(self):
        """LDS bytes one frame of fixed-point layered min-sum takes (-1: the kernel does not take the code)."""
        return int(self.lib.ldpc_hip_layered_fixed_lds_bytes(self.ctx))

    def layered_fixed_direct_lds_bytes(self):
        """LDS bytes one frame of fixed-point layered min-sum takes on float32, float16 or int8 input of decode_batch_typed: no
        binary64 LLRs are staged (-1: the layered plan does not take the code)."""
        return int(self.lib.ldpc_hip_layered_fixed_direct_lds_bytes(self.ctx))

    def philox(self, seed, tag, frame, first_block, n_blocks):
        """The counter mode's raw words, [n_blocks][4] uint32: blocks first_block.. of `frame` under `tag` (0 AWGN, 1 BSC /
        BEC, 2 encoder info bits, 3 the draws of bit_flip_batch, 4 the table of relay_gammas), from the device generator."""
        out = np.zeros((int(n_blocks), 4), np.uint32)
        self._check(self.lib.ldpc_hip_philox(self.ctx, int(seed), int(tag), int(frame), int(first_block), int(n_blocks),
                                             _ptr(out), None), "ldpc_hip_philox")
        return out

    def decode_batch(self, llr_in, early_term=True, iterations=50, decoding="BP",
                     want=("iters", "hard", "llr_out"), out=None, stream=None):
        """Decode llr_in[n][nc] (column order)."""
        n = int(llr_in.shape[0])
        s, bufs = self._outs(n, want, out)
        self._check(self.lib.ldpc_hip_decode_batch(self.ctx, _dec(early_term, iterations, decoding), n, _ptr(llr_in),
                                                   ct.byref(s), stream), "ldpc_hip_decode_batch")
        return bufs

    LLR_TYPES = {"float64": 0, "float32": 1, "float16": 2, "int8": 3}

    def decode_batch_typed(self, llr_in, early_term=True, iterations=50, decoding="BP",
                           want=("iters", "hard", "llr_out"), out=None, stream=None):
        """decode_batch for llr_in[n][nc] of dtype float64, float32, float16 or int8 (a numpy array or a torch tensor, host or
        device; anything else raises TypeError): the outputs are those of decode_batch on the widened values, an int8 k standing
        for k * step of the fixed-point mode in force (include/ldpc_amd.h, ldpc_hip_decode_batch_typed).  "hard_bits" in `want`
        (or a buffer in out["hard_bits"]) gives the decisions packed 32 to a word, uint32 [n][ceil(nc / 32)]."""
        name = str(llr_in.dtype).replace("torch.", "")
        if name not in self.LLR_TYPES:
            raise TypeError(f"decode_batch_typed takes float64, float32, float16 or int8 LLRs, not {llr_in.dtype}")
        n = int(llr_in.shape[0])
        bufs = dict(out or {})
        if "hard_bits" in want and "hard_bits" not in bufs:
            bufs["hard_bits"] = np.zeros((n, (self.nc + 31) // 32), np.uint32)
        s, bufs = self._outs(n, [k for k in want if k != "hard_bits"], bufs)
        self._check(self.lib.ldpc_hip_decode_batch_typed(self.ctx, _dec(early_term, iterations, decoding), n, _ptr(llr_in),
                                                         self.LLR_TYPES[name], ct.byref(s), _ptr(bufs.get("hard_bits")), stream),
                    "ldpc_hip_decode_batch_typed")
        return bufs

    BITS_FORMATS = {"uint8": 0, "uint32": 1}

    def _bits(self, rows, length, what):
        """(frames, format) of rows[n][length bits]: uint8 = a byte per bit, uint32 = packed 32 to a word."""
        name = str(rows.dtype).replace("torch.", "")
        if name not in self.BITS_FORMATS:
            raise TypeError(f"{what} takes uint8 (a byte per bit) or uint32 (packed) rows, not {rows.dtype}")
        width = length if name == "uint8" else (length + 31) // 32
        if len(rows.shape) != 2 or int(rows.shape[1]) != width:
            raise ValueError(f"{what}: rows of {length} bits as {name} are [n][{width}], not {tuple(rows.shape)}")
        return int(rows.shape[0]), self.BITS_FORMATS[name]

    @staticmethod
    def _wanted(want, out, spec):
        """Buffers of the outputs named in `want` (numpy, allocated here) or passed in `out`; spec: name -> (shape, dtype)."""
        bufs = dict(out or {})
        for name in list(want) + list(bufs):
            if name not in spec:
                raise KeyError(f"unknown output {name!r} (one of {sorted(spec)})")
        for name in want:
            if name not in bufs:
                bufs[name] = np.zeros(*spec[name])
        return bufs

    def encode_batch(self, info, want=("codeword",), out=None, stream=None):
        """info[n][kc] -> "codeword" (uint8 [n][nc]) and / or "codeword_bits" (uint32 [n][ceil(nc / 32)]), column order, frame
        by frame u G with no running sum (include/ldpc_amd.h, ldpc_hip_encode_batch).  info is a numpy array or a torch tensor,
        host or device; its dtype tells the format: uint8 = a byte per bit, uint32 = packed (anything else raises TypeError)."""
        n, fmt = self._bits(info, self.kc, "encode_batch")
        bufs = self._wanted(want, out, {"codeword": ((n, self.nc), np.uint8), "codeword_bits": ((n, (self.nc + 31) // 32), np.uint32)})
        self._check(self.lib.ldpc_hip_encode_batch(self.ctx, n, _ptr(info), fmt, _ptr(bufs.get("codeword")),
                                                   _ptr(bufs.get("codeword_bits")), stream), "ldpc_hip_encode_batch")
        return bufs

    def syndrome_batch(self, word, want=("weight",), out=None, stream=None):
        """word[n][nc] (uint8 or packed uint32, column order) -> "syndrome" (uint8 [n][mc]), "syndrome_bits" (uint32
        [n][ceil(mc / 32)]) and "weight" (uint32 [n], the unsatisfied check nodes); include/ldpc_amd.h, ldpc_hip_syndrome_batch."""
        n, fmt = self._bits(word, self.nc, "syndrome_batch")
        bufs = self._wanted(want, out, {"syndrome": ((n, self.mc), np.uint8), "syndrome_bits": ((n, (self.mc + 31) // 32), np.uint32),
                                        "weight": ((n,), np.uint32)})
        self._check(self.lib.ldpc_hip_syndrome_batch(self.ctx, n, _ptr(word), fmt, _ptr(bufs.get("syndrome")),
                                                     _ptr(bufs.get("syndrome_bits")), _ptr(bufs.get("weight")), stream),
                    "ldpc_hip_syndrome_batch")
        return bufs

    def bit_errors_batch(self, a, b, out=None, stream=None):
        """The transmitted positions at which rows f of a[n][nc] and b[n][nc] differ, uint32 [n]; each operand uint8 or packed
        uint32 (include/ldpc_amd.h, ldpc_hip_bit_errors_batch).  `out`: a buffer for the counts (else a numpy array)."""
        n, fa = self._bits(a, self.nc, "bit_errors_batch")
        nb, fb = self._bits(b, self.nc, "bit_errors_batch")
        if n != nb:
            raise ValueError(f"bit_errors_batch: {n} rows against {nb}")
        res = np.zeros(n, np.uint32) if out is None else out
        self._check(self.lib.ldpc_hip_bit_errors_batch(self.ctx, n, _ptr(a), fa, _ptr(b), fb, _ptr(res), stream),
                    "ldpc_hip_bit_errors_batch")
        return res

    def channel_batch(self, codeword, channel, x, seed=0, first_frame=0, bits_per_symbol=1, llr="float64", q_bits=0, step=1.0,
                      frames=None, want=("llr",), out=None, stream=None):
        """codeword[n][nc] (uint8 or packed uint32, column order; None = `frames` all-zero codewords) through the channel
        ("AWGN": x = Es / sigma^2 in dB, 2^bits_per_symbol-ASK; "BSC": x = the crossover probability) under the counter noise of
        (seed, first_frame + row) -> "llr" ([n][nc] of dtype `llr`: float64, float32, float16, or int8 with q_bits and step)
        and / or "received" (float64 [n][ceil(nct / bits_per_symbol)]); include/ldpc_amd.h, ldpc_hip_channel_batch.  codeword
        and the buffers in `out` are numpy arrays or torch tensors, host or device; a wrong dtype raises TypeError, a wrong shape
        ValueError."""
        if llr not in self.LLR_TYPES:
            raise TypeError(f"channel_batch writes float64, float32, float16 or int8 LLRs, not {llr!r}")
        if codeword is None:
            if frames is None:
                raise ValueError("channel_batch: codeword=None (all-zero codewords) needs frames=")
            n, fmt = int(frames), 0
        else:
            n, fmt = self._bits(codeword, self.nc, "channel_batch")
            if frames is not None and int(frames) != n:
                raise ValueError(f"channel_batch: frames={frames} against {n} rows")
        m = int(bits_per_symbol)
        symbols = -(-self.nct // m) if 1 <= m <= 4 else 0  # (the library refuses other m)
        spec = {"llr": ((n, self.nc), np.dtype(llr)), "received": ((n, symbols), np.float64)}
        bufs = self._wanted(want, out, spec)
        for name, buf in bufs.items():
            shape, dt = spec[name]
            if str(buf.dtype).replace("torch.", "") != np.dtype(dt).name:
                raise TypeError(f"channel_batch: {name} is {np.dtype(dt).name}, not {buf.dtype}")
            if tuple(buf.shape) != shape:
                raise ValueError(f"channel_batch: {name} is {shape}, not {tuple(buf.shape)}")
        ch = ldpc_hip_channel(CHANNELS[channel] if isinstance(channel, str) else int(channel), float(x), int(seed), int(first_frame),
                              m, self.LLR_TYPES[llr], int(q_bits), float(step))
        self._check(self.lib.ldpc_hip_channel_batch(self.ctx, ct.byref(ch), n, _ptr(codeword), fmt, _ptr(bufs.get("llr")),
                                                    _ptr(bufs.get("received")), stream), "ldpc_hip_channel_batch")
        return bufs

    def _check_bufs(self, what, bufs, spec):
        for name, buf in bufs.items():
            shape, dt = spec[name]
            if str(buf.dtype).replace("torch.", "") != np.dtype(dt).name:
                raise TypeError(f"{what}: {name} is {np.dtype(dt).name}, not {buf.dtype}")
            if tuple(buf.shape) != shape:
                raise ValueError(f"{what}: {name} is {shape}, not {tuple(buf.shape)}")

    def erasure_channel_batch(self, codeword, eps, seed=0, first_frame=0, frames=None, want=("word", "erased"), out=None, stream=None):
        """codeword[n][nc] (uint8 or packed uint32, column order; None = `frames` all-zero codewords) through the erasure channel
        of probability eps under the counter noise of (seed, first_frame + row) -> "word" and / or "erased", both packed uint32
        [n][ceil(nc / 32)]: erased marks the holes (punctured columns always), word is the codeword where it is not erased
        (include/ldpc_amd.h, ldpc_hip_erasure_channel_batch).  codeword and the buffers in `out` are numpy arrays or torch
        tensors, host or device; a wrong dtype raises TypeError, a wrong shape ValueError."""
        if codeword is None:
            if frames is None:
                raise ValueError("erasure_channel_batch: codeword=None (all-zero codewords) needs frames=")
            n, fmt = int(frames), 0
        else:
            n, fmt = self._bits(codeword, self.nc, "erasure_channel_batch")
            if frames is not None and int(frames) != n:
                raise ValueError(f"erasure_channel_batch: frames={frames} against {n} rows")
        packed = ((n, (self.nc + 31) // 32), np.uint32)
        spec = {"word": packed, "erased": packed}
        bufs = self._wanted(want, out, spec)
        self._check_bufs("erasure_channel_batch", bufs, spec)
        self._check(self.lib.ldpc_hip_erasure_channel_batch(self.ctx, float(eps), int(seed), int(first_frame), n, _ptr(codeword), fmt,
                                                            _ptr(bufs.get("word")), _ptr(bufs.get("erased")), stream),
                    "ldpc_hip_erasure_channel_batch")
        return bufs

    ERASURE_EARLY_TERM, ERASURE_STOP_STALLED = 1, 2

    def erasure_decode_batch(self, word, erased, iterations=50, early_term=True, stop_stalled=False,
                             want=("word", "erased", "iters", "unresolved"), out=None, stream=None):
        """word[n][nc] and erased[n][nc] (both uint8 or both packed uint32) -> what peeling recovers: "word" and "erased" (packed
        uint32 [n][ceil(nc / 32)]: the values and the holes that are left), "iters" and "unresolved" (uint32 [n]: passes, holes
        left).  No generator and no codeword is needed.  early_term: a frame without holes stops; stop_stalled: so does one whose
        pass filled none (include/ldpc_amd.h, ldpc_hip_erasure_decode_batch).  Inputs and the buffers in `out` are numpy arrays
        or torch tensors, host or device."""
        n, fmt = self._bits(word, self.nc, "erasure_decode_batch")
        ne, fe = self._bits(erased, self.nc, "erasure_decode_batch")
        if (n, fmt) != (ne, fe):
            raise ValueError(f"erasure_decode_batch: word is {tuple(word.shape)} {word.dtype}, erased is {tuple(erased.shape)} {erased.dtype}")
        packed = ((n, (self.nc + 31) // 32), np.uint32)
        spec = {"word": packed, "erased": packed, "iters": ((n,), np.uint32), "unresolved": ((n,), np.uint32)}
        bufs = self._wanted(want, out, spec)
        self._check_bufs("erasure_decode_batch", bufs, spec)
        flags = (self.ERASURE_EARLY_TERM if early_term else 0) | (self.ERASURE_STOP_STALLED if stop_stalled else 0)
        self._check(self.lib.ldpc_hip_erasure_decode_batch(self.ctx, int(iterations), flags, n, _ptr(word), _ptr(erased), fmt,
                                                           _ptr(bufs.get("word")), _ptr(bufs.get("erased")), _ptr(bufs.get("iters")),
                                                           _ptr(bufs.get("unresolved")), stream), "ldpc_hip_erasure_decode_batch")
        return bufs

    def erasure_lds_bytes(self):
        """LDS bytes one 32-frame group of erasure_decode_batch takes (-1: the decoder does not take the code)."""
        return int(self.lib.ldpc_hip_erasure_lds_bytes(self.ctx))

    ERASURE_SOLVED, ERASURE_PARTIAL, ERASURE_INCONSISTENT, ERASURE_TOO_LARGE = 0, 1, 2, 3

    def erasure_solve_batch(self, word, erased, max_unknowns=None, want=("word", "erased", "unresolved", "rank", "status"), out=None,
                            stream=None):
        """word[n][nc] and erased[n][nc] (both uint8 or both packed uint32) -> every erased bit that the parity checks determine,
        by elimination over GF(2): "word" and "erased" (packed uint32 [n][ceil(nc / 32)]: the values and the holes that are left),
        "unresolved", "rank" and "status" (uint32 [n]: holes left, rank of the erased columns, ERASURE_SOLVED / _PARTIAL /
        _INCONSISTENT / _TOO_LARGE); include/ldpc_amd.h, ldpc_hip_erasure_solve_batch.  A frame with more than max_unknowns holes
        comes back as it is; None = the largest cap that fits the LDS of a CU.  Advised: erasure_decode_batch(stop_stalled=True)
        first, this call on what it leaves.  Inputs and the buffers in `out` are numpy arrays or torch tensors, host or device; a
        wrong dtype raises TypeError, a wrong shape ValueError."""
        n, fmt = self._bits(word, self.nc, "erasure_solve_batch")
        ne, fe = self._bits(erased, self.nc, "erasure_solve_batch")
        if (n, fmt) != (ne, fe):
            raise ValueError(f"erasure_solve_batch: word is {tuple(word.shape)} {word.dtype}, erased is {tuple(erased.shape)} {erased.dtype}")
        packed = ((n, (self.nc + 31) // 32), np.uint32)
        spec = {"word": packed, "erased": packed, "unresolved": ((n,), np.uint32), "rank": ((n,), np.uint32), "status": ((n,), np.uint32)}
        bufs = self._wanted(want, out, spec)
        self._check_bufs("erasure_solve_batch", bufs, spec)
        cap = (self.erasure_solve_max_unknowns() or 1) if max_unknowns is None else int(max_unknowns)  # (1: refused for its LDS)
        if not 0 <= cap < 2**32:
            raise ValueError(f"erasure_solve_batch: max_unknowns={max_unknowns}")
        self._check(self.lib.ldpc_hip_erasure_solve_batch(self.ctx, cap, n, _ptr(word), _ptr(erased), fmt, _ptr(bufs.get("word")),
                                                          _ptr(bufs.get("erased")), _ptr(bufs.get("unresolved")), _ptr(bufs.get("rank")),
                                                          _ptr(bufs.get("status")), stream), "ldpc_hip_erasure_solve_batch")
        return bufs

    def erasure_solve_lds_bytes(self, max_unknowns):
        """LDS bytes one frame of erasure_solve_batch takes at that cap (-1: it does not fit a CU, or the cap is 0)."""
        return int(self.lib.ldpc_hip_erasure_solve_lds_bytes(self.ctx, int(max_unknowns)))

    def erasure_solve_max_unknowns(self):
        """The largest max_unknowns erasure_solve_batch takes on this code (the LDS is monotone in it); 0 if none fits."""
        if self.erasure_solve_lds_bytes(self.nc) >= 0:
            return self.nc
        lo, hi = 0, self.nc  # lo fits (or is 0), hi does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if self.erasure_solve_lds_bytes(mid) >= 0 else (lo, mid)
        return lo

    OSD_CODEWORD, OSD_ORDER0, OSD_REPROCESSED, OSD_NO_COLUMN = 0, 1, 2, 0xFFFFFFFF

    def osd_batch(self, llr, candidates=0, want=("word", "flips", "metric", "flipped_column", "status"), out=None, stream=None):
        """llr[n][nc] (float64, float32, float16 or int8, column order; a decoder's llr_out for BP + OSD) -> the codeword of
        ordered-statistics decoding: order 0 on the most reliable independent columns, then the best of the first `candidates`
        single flips among them.  "word" (packed uint32 [n][ceil(nc / 32)], always a codeword), "flips" (uint32 [n]: the columns
        where it leaves the hard decisions), "metric" (uint64 [n]: their reliabilities summed), "flipped_column" (uint32 [n]:
        the column of the winning flip, OSD_NO_COLUMN if none) and "status" (uint32 [n]: OSD_CODEWORD / _ORDER0 / _REPROCESSED);
        include/ldpc_amd.h, ldpc_hip_osd_batch.  llr and the buffers in `out` are numpy arrays or torch tensors, host or device;
        a wrong dtype raises TypeError, a wrong shape ValueError."""
        name = str(llr.dtype).replace("torch.", "")
        if name not in self.LLR_TYPES:
            raise TypeError(f"osd_batch takes float64, float32, float16 or int8 LLRs, not {llr.dtype}")
        if len(llr.shape) != 2 or int(llr.shape[1]) != self.nc:
            raise ValueError(f"osd_batch: llr is [n][{self.nc}], not {tuple(llr.shape)}")
        if not 0 <= int(candidates) < 2**32:
            raise ValueError(f"osd_batch: candidates={candidates}")
        n = int(llr.shape[0])
        spec = {"word": ((n, (self.nc + 31) // 32), np.uint32), "flips": ((n,), np.uint32), "metric": ((n,), np.uint64),
                "flipped_column": ((n,), np.uint32), "status": ((n,), np.uint32)}
        bufs = self._wanted(want, out, spec)
        self._check_bufs("osd_batch", bufs, spec)
        self._check(self.lib.ldpc_hip_osd_batch(self.ctx, int(candidates), n, _ptr(llr), self.LLR_TYPES[name], _ptr(bufs.get("word")),
                                                _ptr(bufs.get("flips")), _ptr(bufs.get("metric")), _ptr(bufs.get("flipped_column")),
                                                _ptr(bufs.get("status")), stream), "ldpc_hip_osd_batch")
        return bufs

    def osd_lds_bytes(self):
        """LDS bytes one frame of osd_batch takes (-1: the check matrix does not fit a CU, and osd_batch refuses the code)."""
        return int(self.lib.ldpc_hip_osd_lds_bytes(self.ctx))

    OSD_REPROCESSED_PAIR, OSD_INFEASIBLE = 3, 4

    def osd_syndrome_batch(self, llr, syndrome=None, candidates=0, pair_depth=0,
                           want=("word", "flips", "metric", "flipped_columns", "status"), out=None, stream=None):
        """Ordered-statistics decoding toward a given syndrome: llr[n][nc] as in osd_batch, syndrome[n][mc] as in
        syndrome_decode_batch (uint8, or packed uint32 as syndrome_batch writes it; None = all zero) -> the word x with
        H x = syndrome that keeps the hard decisions on the most reliable independent columns, the best of the first
        `candidates` single flips among them and of every pair among the first `pair_depth` (at most 256) of them.  "word",
        "flips", "metric" as in osd_batch; "flipped_columns" (uint32 [n][2]: the winning flip's columns, OSD_NO_COLUMN where
        there is none) and "status" (uint32 [n]: OSD_CODEWORD = the decisions already meet the syndrome, OSD_ORDER0,
        OSD_REPROCESSED, OSD_REPROCESSED_PAIR, or OSD_INFEASIBLE = no word has this syndrome, and "word" is the decisions);
        include/ldpc_amd.h, ldpc_hip_osd_syndrome_batch.  Inputs and the buffers in `out` are numpy arrays or torch tensors,
        host or device; a wrong dtype raises TypeError, a wrong shape ValueError."""
        name = str(llr.dtype).replace("torch.", "")
        if name not in self.LLR_TYPES:
            raise TypeError(f"osd_syndrome_batch takes float64, float32, float16 or int8 LLRs, not {llr.dtype}")
        if len(llr.shape) != 2 or int(llr.shape[1]) != self.nc:
            raise ValueError(f"osd_syndrome_batch: llr is [n][{self.nc}], not {tuple(llr.shape)}")
        n, fmt = int(llr.shape[0]), 0
        if syndrome is not None:
            ns, fmt = self._bits(syndrome, self.mc, "osd_syndrome_batch")
            if ns != n:
                raise ValueError(f"osd_syndrome_batch: {n} rows of llr against {ns} of syndrome")
        if not 0 <= int(candidates) < 2**32 or not 0 <= int(pair_depth) < 2**32:
            raise ValueError(f"osd_syndrome_batch: candidates={candidates}, pair_depth={pair_depth}")
        spec = {"word": ((n, (self.nc + 31) // 32), np.uint32), "flips": ((n,), np.uint32), "metric": ((n,), np.uint64),
                "flipped_columns": ((n, 2), np.uint32), "status": ((n,), np.uint32)}
        bufs = self._wanted(want, out, spec)
        self._check_bufs("osd_syndrome_batch", bufs, spec)
        self._check(self.lib.ldpc_hip_osd_syndrome_batch(self.ctx, int(candidates), int(pair_depth), n, _ptr(llr), self.LLR_TYPES[name],
                                                         _ptr(syndrome), fmt, _ptr(bufs.get("word")), _ptr(bufs.get("flips")),
                                                         _ptr(bufs.get("metric")), _ptr(bufs.get("flipped_columns")),
                                                         _ptr(bufs.get("status")), stream), "ldpc_hip_osd_syndrome_batch")
        return bufs

    def osd_syndrome_lds_bytes(self):
        """LDS bytes one frame of osd_syndrome_batch takes (-1: the check matrix does not fit a CU, and the call refuses the code)."""
        return int(self.lib.ldpc_hip_osd_syndrome_lds_bytes(self.ctx))

    SYNDROME_SHARED_LLR = 1

    def syndrome_decode_batch(self, llr, syndrome=None, iterations=50, early_term=True, q_bits=6, step=0.25, scale=1.0, offset=0.0,
                              shared_llr=False, want=("hard_bits", "iters", "weight"), out=None, stream=None):
        """Quantized min-sum decoding toward a given syndrome: the word x with H x = syndrome that fits llr[n][nc] (float64,
        float32, float16 or int8, column order; all nc columns are the caller's).  syndrome[n][mc] is uint8 (a byte per check
        node) or packed uint32 [n][ceil(mc / 32)], what syndrome_batch writes; None = all zero.  shared_llr: llr is one row
        [nc] (or [1][nc]) used for every frame, the frames counted by the syndrome's rows.  Messages of q_bits bits (2..8) with
        LLR step `step` and the correction (scale, offset); nothing is read from the context's settings.  "hard_bits" (packed
        uint32 [n][ceil(nc / 32)]), "iters" and "weight" (uint32 [n]: the iteration that reached the syndrome, the check nodes
        the returned word leaves unmet: 0 iff it has the syndrome) and "llr_out" (float64 [n][nc]); iterations=0 returns the
        quantized input.  include/ldpc_amd.h, ldpc_hip_syndrome_decode_batch.  Inputs and the buffers in `out` are numpy
        arrays or torch tensors, host or device; a wrong dtype raises TypeError, a wrong shape ValueError."""
        who = "syndrome_decode_batch"
        kind, n, fmt, bufs = self._syndrome_decode_call(who, llr, syndrome, shared_llr, iterations, want, out)
        p = ldpc_hip_syndrome_decode(int(iterations), int(bool(early_term)), int(q_bits), float(step), float(scale), float(offset),
                                     self.SYNDROME_SHARED_LLR if shared_llr else 0)
        self._check(self.lib.ldpc_hip_syndrome_decode_batch(self.ctx, ct.byref(p), n, _ptr(llr), kind, _ptr(syndrome), fmt,
                                                            _ptr(bufs.get("hard_bits")), _ptr(bufs.get("iters")), _ptr(bufs.get("weight")),
                                                            _ptr(bufs.get("llr_out")), stream), "ldpc_hip_syndrome_decode_batch")
        return bufs

    def _syndrome_decode_call(self, who, llr, syndrome, shared_llr, iterations, want, out, further=None):
        """What the decoders toward a syndrome check of their arguments before the library sees them -> the LLR type, the
        frames, the syndrome's format and the output buffers.  `further`: the names of uint32 [n] outputs that take the place
        of llr_out."""
        name = str(llr.dtype).replace("torch.", "")
        if name not in self.LLR_TYPES:
            raise TypeError(f"{who} takes float64, float32, float16 or int8 LLRs, not {llr.dtype}")
        fmt = 0
        if syndrome is not None:
            ns, fmt = self._bits(syndrome, self.mc, who)
        if shared_llr:
            if tuple(llr.shape) not in ((self.nc,), (1, self.nc)):
                raise ValueError(f"{who}: a shared llr is [{self.nc}] or [1][{self.nc}], not {tuple(llr.shape)}")
            if syndrome is None:
                raise ValueError(f"{who}: shared_llr needs a syndrome (its rows count the frames)")
            n = ns
        else:
            if len(llr.shape) != 2 or int(llr.shape[1]) != self.nc:
                raise ValueError(f"{who}: llr is [n][{self.nc}], not {tuple(llr.shape)}")
            n = int(llr.shape[0])
            if syndrome is not None and ns != n:
                raise ValueError(f"{who}: {n} rows of llr against {ns} of syndrome")
        if not 0 <= int(iterations) < 2**32:
            raise ValueError(f"{who}: iterations={iterations}")
        spec = {"hard_bits": ((n, (self.nc + 31) // 32), np.uint32), "iters": ((n,), np.uint32), "weight": ((n,), np.uint32),
                "llr_out": ((n, self.nc), np.float64)}
        if further is not None:
            del spec["llr_out"]
            spec.update({k: ((n,), np.uint32) for k in further})
        bufs = self._wanted(want, out, spec)
        self._check_bufs(who, bufs, spec)
        return self.LLR_TYPES[name], n, fmt, bufs

    def syndrome_decode_lds_bytes(self):
        """LDS bytes one frame of syndrome_decode_batch takes (-1: the call does not take the code)."""
        return int(self.lib.ldpc_hip_syndrome_decode_lds_bytes(self.ctx))

    def syndrome_decode_layered_batch(self, llr, syndrome=None, iterations=50, early_term=True, msg_bits=6, app_bits=8, step=0.25,
                                      scale=1.0, offset=0.0, shared_llr=False, want=("hard_bits", "iters", "weight"), out=None,
                                      stream=None):
        """syndrome_decode_batch on the layered (row-serial) schedule in fixed point: messages of msg_bits bits (2..8), saturating
        totals of app_bits bits (msg_bits..16), LLR step `step` and the correction (scale, offset); about half the sweeps of the
        flooding call, and "iters" counts sweeps.  Arguments, outputs and buffers as there; nothing is read from the context's
        settings; iterations=0 returns the quantized input.  Takes the codes of the layered schedule (check nodes of degree
        2..8).  include/ldpc_amd.h, ldpc_hip_syndrome_decode_layered_batch."""
        who = "syndrome_decode_layered_batch"
        kind, n, fmt, bufs = self._syndrome_decode_call(who, llr, syndrome, shared_llr, iterations, want, out)
        p = ldpc_hip_syndrome_decode_layered(int(iterations), int(bool(early_term)), int(msg_bits), int(app_bits), float(step), float(scale),
                                             float(offset), self.SYNDROME_SHARED_LLR if shared_llr else 0)
        self._check(self.lib.ldpc_hip_syndrome_decode_layered_batch(self.ctx, ct.byref(p), n, _ptr(llr), kind, _ptr(syndrome), fmt,
                                                                    _ptr(bufs.get("hard_bits")), _ptr(bufs.get("iters")),
                                                                    _ptr(bufs.get("weight")), _ptr(bufs.get("llr_out")), stream),
                    "ldpc_hip_syndrome_decode_layered_batch")
        return bufs

    def syndrome_decode_layered_lds_bytes(self):
        """LDS bytes one frame of syndrome_decode_layered_batch takes (-1: the call does not take the code)."""
        return int(self.lib.ldpc_hip_syndrome_decode_layered_lds_bytes(self.ctx))

    def bit_flip_batch(self, llr, syndrome=None, *, iterations=50, q_bits=2, step=1.0, check_weight=2, margin=0, flip_prob=1.0, seed=0,
                       first_frame=0, shared_llr=False, want=("hard_bits", "iters", "weight"), out=None, stream=None):
        """Gradient-descent bit flipping toward a given syndrome: in each of at most `iterations` rounds every column within
        `margin` of the frame's largest penalty check_weight * (unmet check nodes of the column) +- (its reliability, + where
        the bit differs from the input's decision) flips; with flip_prob < 1 each such column flips with that probability
        (PGDBF), drawn from Philox under tag 3, `seed` and frame index first_frame + f.  Reliabilities of q_bits bits (2..8)
        with LLR step `step`; hard decisions are int8 +-1 with q_bits=2.  llr, syndrome, shared_llr, "hard_bits", "iters" (the
        rounds run) and "weight" as in syndrome_decode_batch; there is no "llr_out".  flip_prob 1.0 is the threshold
        0xFFFFFFFF (no draws), any other value floor(flip_prob * 2^32).  include/ldpc_amd.h, ldpc_hip_bit_flip_batch."""
        who = "bit_flip_batch"
        if "llr_out" in tuple(want) or "llr_out" in (out or {}):
            raise ValueError(f"{who}: there is no llr_out (outputs: hard_bits, iters, weight)")
        if not 0.0 <= float(flip_prob) <= 1.0:
            raise ValueError(f"{who}: flip_prob={flip_prob} is outside [0, 1]")
        for name, v in (("check_weight", check_weight), ("margin", margin)):
            if not 0 <= int(v) < 2**32:
                raise ValueError(f"{who}: {name}={v}")
        for name, v in (("seed", seed), ("first_frame", first_frame)):
            if not 0 <= int(v) < 2**64:
                raise ValueError(f"{who}: {name}={v}")
        kind, n, fmt, bufs = self._syndrome_decode_call(who, llr, syndrome, shared_llr, iterations, want, out)
        threshold = 0xFFFFFFFF if float(flip_prob) == 1.0 else int(float(flip_prob) * 2.0**32)  # (exact: a power of two)
        p = ldpc_hip_bit_flip(int(iterations), int(q_bits), float(step), int(check_weight), int(margin), threshold, int(seed),
                              int(first_frame), self.SYNDROME_SHARED_LLR if shared_llr else 0)
        self._check(self.lib.ldpc_hip_bit_flip_batch(self.ctx, ct.byref(p), n, _ptr(llr), kind, _ptr(syndrome), fmt,
                                                     _ptr(bufs.get("hard_bits")), _ptr(bufs.get("iters")), _ptr(bufs.get("weight")), stream),
                    "ldpc_hip_bit_flip_batch")
        return bufs

    def bit_flip_lds_bytes(self):
        """LDS bytes one frame of bit_flip_batch takes (-1: the call does not take the code)."""
        return int(self.lib.ldpc_hip_bit_flip_lds_bytes(self.ctx))

    RELAY_OUTPUTS = ("hard_bits", "iters", "weight", "solutions", "best_leg", "cost")
    RELAY_NONE, TAG_RELAY = 0xFFFFFFFF, 4

    def relay_decode_batch(self, llr, syndrome=None, gamma=None, *, legs, first_iterations=50, leg_iterations=30, stop_after=1, q_bits=6,
                           step=0.25, scale=1.0, offset=0.0, form=0, shared_llr=False, want=RELAY_OUTPUTS, out=None, stream=None):
        """Min-sum with memory, run as a relay of `legs` legs, toward a given syndrome: the decoder for degenerate codes
        (quantum LDPC, surface codes) on which syndrome_decode_batch swings between solutions.  In every iteration a column's
        prior is its input plus gamma[leg][column] / 64 times (its previous total - its input); leg 0 may take
        first_iterations, every later leg leg_iterations, each starts from the totals the last one left; every word that meets
        the syndrome is priced by the input magnitudes it contradicts, the cheapest is returned, and a frame ends once
        stop_after legs have met the syndrome.  gamma is int8 [legs][nc] in column order, host or device, shared by all frames
        (None = all zero; relay_gammas draws one).  llr, syndrome, shared_llr, q_bits, step, scale, offset as in
        syndrome_decode_batch.  form: 0 = the library chooses, 1 = a workgroup per frame, 2 = a wave per frame (same results).
        "hard_bits", "iters" (summed over the legs run) and "weight" as there; "solutions" (the legs that met the syndrome),
        "best_leg" and "cost" (those of the returned word, RELAY_NONE where no leg met it), all uint32 [n].
        include/ldpc_amd.h, ldpc_hip_relay_decode_batch."""
        who = "relay_decode_batch"
        for name, v in (("legs", legs), ("first_iterations", first_iterations), ("leg_iterations", leg_iterations), ("stop_after", stop_after)):
            if not 0 <= int(v) < 2**32:
                raise ValueError(f"{who}: {name}={v}")
        if gamma is not None:
            if str(gamma.dtype).replace("torch.", "") != "int8":
                raise TypeError(f"{who}: gamma is int8, not {gamma.dtype}")
            if tuple(gamma.shape) != (int(legs), self.nc):
                raise ValueError(f"{who}: gamma is [{int(legs)}][{self.nc}], not {tuple(gamma.shape)}")
        kind, n, fmt, bufs = self._syndrome_decode_call(who, llr, syndrome, shared_llr, 0, want, out, further=self.RELAY_OUTPUTS[3:])
        p = ldpc_hip_relay_decode(int(legs), int(first_iterations), int(leg_iterations), int(stop_after), int(q_bits), float(step),
                                  float(scale), float(offset), int(form), self.SYNDROME_SHARED_LLR if shared_llr else 0)
        self._check(self.lib.ldpc_hip_relay_decode_batch(self.ctx, ct.byref(p), n, _ptr(llr), kind, _ptr(syndrome), fmt, _ptr(gamma),
                                                         *(_ptr(bufs.get(k)) for k in self.RELAY_OUTPUTS), stream),
                    "ldpc_hip_relay_decode_batch")
        return bufs

    def relay_decode_lds_bytes(self, form=0):
        """LDS bytes one frame of relay_decode_batch takes in `form` (-1: the call does not take the code in that form)."""
        return int(self.lib.ldpc_hip_relay_decode_lds_bytes(self.ctx, int(form)))

    def relay_gammas(self, legs, lo, hi, seed, first=0):
        """A gamma table for relay_decode_batch, int8 [legs][nc]: row 0 is `first` everywhere; row l >= 1, column v is
        lo + ((draw * (hi - lo + 1)) >> 32), the draw being word v & 3 of Philox block v >> 2 of frame l under tag 4 and `seed`
        (the device generator: philox)."""
        if not (1 <= int(legs) <= 256 and -128 <= int(lo) <= int(hi) <= 127 and -128 <= int(first) <= 127):
            raise ValueError(f"relay_gammas: legs={legs}, lo={lo}, hi={hi}, first={first}")
        g = np.full((int(legs), self.nc), int(first), np.int8)
        for leg in range(1, int(legs)):
            draw = self.philox(seed, self.TAG_RELAY, leg, 0, (self.nc + 3) // 4).reshape(-1)[:self.nc].astype(np.uint64)
            g[leg] = (int(lo) + ((draw * np.uint64(int(hi) - int(lo) + 1)) >> np.uint64(32)).astype(np.int64)).astype(np.int8)
        return g

    def stream_begin(self, channel, seed, x):
        """Channel point x of mt19937_64(seed); also resets the encoder (a fresh channel object)."""
        ch = CHANNELS[channel] if isinstance(channel, str) else int(channel)
        self._check(self.lib.ldpc_hip_stream_begin(self.ctx, ch, int(seed), float(x)), "ldpc_hip_stream_begin")

    def stream_skip(self, n, stream=None):
        self._check(self.lib.ldpc_hip_stream_skip(self.ctx, int(n), stream), "ldpc_hip_stream_skip")

    def stream_decode(self, n, early_term=True, iterations=50, decoding="BP", want=("iters", "bit_errors"),
                      out=None, stream=None):
        s, bufs = self._outs(int(n), want, out)
        self._check(self.lib.ldpc_hip_stream_decode(self.ctx, _dec(early_term, iterations, decoding), int(n),
                                                    ct.byref(s), stream), "ldpc_hip_stream_decode")
        return bufs

    def shard_capacity(self, target_frames, world):
        return int(self.lib.ldpc_hip_shard_capacity(self.ctx, int(target_frames), int(world)))

    def stream_decode_sharded(self, comm, target_frames, early_term=True, iterations=50, decoding="BP",
                              want=("iters", "bit_errors"), out=None, stream=None):
        """This rank's share of the next global step of about target_frames frames (every rank calls it).  Returns
        (buffers, step) with step = (step_first, step_frames, first, n); only the first n entries of the buffers are
        this rank's frames."""
        cap = self.shard_capacity(target_frames, comm.world)
        s, bufs = self._outs(cap, want, out)
        step = (ct.c_uint64 * 4)()
        self._check(self.lib.ldpc_hip_stream_decode_sharded(self.ctx, comm.handle, _dec(early_term, iterations, decoding),
                                                            int(target_frames), ct.byref(s), step, stream),
                    "ldpc_hip_stream_decode_sharded")
        return bufs, tuple(int(v) for v in step)

    @property
    def stream_frame(self):
        return self.lib.ldpc_hip_stream_frame(self.ctx)

    @property
    def stream_raw_draws(self):
        n = self.lib.ldpc_hip_stream_raw_draws(self.ctx)
        if n == 2**64 - 1:
            raise RuntimeError("ldpc_hip_stream_raw_draws: " + self.lib.ldpc_hip_last_error().decode())
        return n

    @property
    def jump_tasks(self):
        """jump-ahead tasks the context's noise stream has launched so far"""
        return self.lib.ldpc_hip_jump_tasks(self.ctx)

    def synchronize(self, stream=None):
        self._check(self.lib.ldpc_hip_synchronize(self.ctx, stream), "ldpc_hip_synchronize")

    def set_profiling(self, on=True):
        self.lib.ldpc_hip_set_profiling(self.ctx, int(on))

    def last_ms(self, which=0):
        return float(self.lib.ldpc_hip_last_ms(self.ctx, which))

    def batch_counters(self, iters_ptr, bit_errors_ptr, n, max_iters, early_term, counters_ptr, stream=None):
        """{frames, frame errors, bit errors, iterations, early stops} of a batch, summed on the device (all three
        arguments are device pointers, e.g. tensor.data_ptr()); one launch on `stream`."""
        self._check(self.lib.ldpc_hip_batch_counters(self.ctx, iters_ptr, bit_errors_ptr, int(n), int(max_iters),
                                                     int(bool(early_term)), counters_ptr, stream), "ldpc_hip_batch_counters")

    def selftest_division(self, n, seed=1):
        """Pairs (of n) on which the kernels' division sequence and the IEEE division disagree (expected 0)."""
        bad = ct.c_uint64(0)
        self._check(self.lib.ldpc_hip_selftest_division(self.ctx, int(n), int(seed), ct.byref(bad)),
                    "ldpc_hip_selftest_division")
        return bad.value

    MATH_FNS = ("exp", "log", "boxplus", "ratio_div", "ratio_rho", "ratio_lambda", "e_combine", "exp_clamped", "boxplus_exp",
                "boxplus_log", "cn_ratio3", "cn_ratio4", "cn_ratio5", "cn_ratio6", "cn_ratio8", "cn_llr4", "cn_llr6", "cn_ratio3s", "cn_ratio4s", "cn_ratio6s",
                "cnf2", "cnf3", "cnf4", "cnf3d", "cnf4d", "cn_llr3", "cn_llr5", "cn_llr16", "predicates")

    def selftest_math(self, fn, a, b=None):
        """The device arithmetic of detmath.h / device_cn.hpp on host arrays: fn is a name of MATH_FNS."""
        a = np.ascontiguousarray(a, np.float64)
        out = np.empty_like(a)
        n = a.shape[0]
        bb = None if b is None else np.ascontiguousarray(b, np.float64)
        self._check(self.lib.ldpc_hip_selftest_math(self.ctx, self.MATH_FNS.index(fn), n, _ptr(a), _ptr(bb), _ptr(out)),
                    "ldpc_hip_selftest_math")
        return out

    def mt64(self, seed, first, n):
        out = np.zeros(int(n), np.uint64)
        self._check(self.lib.ldpc_hip_mt64(self.ctx, int(seed), int(first), int(n), _ptr(out), None), "ldpc_hip_mt64")
        return out

    def simulate(self, channel, x_range, seed=0, early_term=True, iterations=50, decoding="BP",
                 max_frames=10**10, fec=50, result_file="", cli_output=False, comm=None):
        n_max = max(1, int(np.ceil((x_range[1] - x_range[0]) / x_range[2])) + 2)
        arrs = {k: np.zeros(n_max, np.float64) for k in ("fer", "ber", "avg_iter", "time")}
        arrs["fec"] = np.zeros(n_max, np.uint64)
        arrs["frames"] = np.zeros(n_max, np.uint64)
        res = sim_results_t(*[arrs[k].ctypes.data_as(ct.POINTER(ct.c_double if arrs[k].dtype == np.float64
                                                                 else ct.c_uint64))
                              for k in ("fer", "ber", "avg_iter", "time", "fec", "frames")])
        totals = np.zeros(4 * n_max, np.uint64)
        stop = ct.c_bool(False)
        ch = channel_param(int(seed), (ct.c_double * 3)(*x_range), channel.encode())
        sp = simulation_param(1, int(max_frames), int(fec), result_file.encode())
        if comm is not None:
            nx = self.lib.ldpc_hip_simulate_sharded(self.ctx, comm.handle, _dec(early_term, iterations, decoding), ch, sp,
                                                    ct.byref(res), totals.ctypes.data, ct.byref(stop), int(cli_output))
        else:
            nx = self.lib.ldpc_hip_simulate(self.ctx, _dec(early_term, iterations, decoding), ch, sp, ct.byref(res),
                                            totals.ctypes.data, ct.byref(stop), int(cli_output))
        if nx < 0:
            raise RuntimeError("ldpc_hip_simulate: " + self.lib.ldpc_hip_last_error().decode())
        out = {k: v[:nx] for k, v in arrs.items()}
        out["totals"] = totals[:4 * nx].reshape(nx, 4)
        return out
