"""GbpEngine — Python face of the device half of the C-ABI: the reference's Poplar program list
(ba.cpp:925-934, slam.cpp:937-948) as methods.  Every call goes through libgbp_mi355x.so (HIP);
construction raises if the library or a GPU is missing — there is no CPU path."""
import ctypes as C

import numpy as np

from . import _cabi as cabi
from ._lib import load


class GbpError(RuntimeError):
    pass


class GbpEngine:
    def __init__(self, cam_id, lmk_id, n_cams, n_lmks, K9, params=None, shard=None, hooks=False):
        """hooks=True loads libgbp_mi355x_test.so — the product sources + the gbp_debug_* test hooks
        (include/gbp_mi355x_debug.h) — instead of the product library; only tests and profiles/ ask for it."""
        self.hooks = hooks if hooks == "exp" else bool(hooks)     # "exp": the experiments build (has the hooks too)
        self.lib = load(hooks=self.hooks)
        self._keep = []
        self.problem = cabi.make_problem(cam_id, lmk_id, n_cams, n_lmks, K9, self._keep)
        self.C, self.L, self.E = int(n_cams), int(n_lmks), int(self.problem.n_edges)
        self.params = params if params is not None else cabi.GbpParams.defaults()
        self.shard = None
        if shard is not None:
            self.shard = cabi.GbpShard(int(shard[0]), int(shard[1]), int(shard[2]), int(shard[3]))
        h = C.c_void_p()
        rc = self.lib.gbp_create(C.byref(self.problem), C.byref(self.params),
                                 C.byref(self.shard) if self.shard is not None else None, C.byref(h))
        if rc != 0:
            raise GbpError("gbp_create: %s (status %d)" % (self.lib.gbp_last_error(None).decode(), rc))
        self.h = h
        self._stream = None          # the caller's stream the ctx runs on (set_stream); None: a stream of the ctx's own
        self._edge_ids = None        # cam_id / lmk_id on the GPU (solution())
        self._device = self._current_device(only_if_initialised=True)      # the GPU the ctx lives on: the current device of gbp_create

    def close(self):
        if getattr(self, "h", None):
            self.lib.gbp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise GbpError("%s: %s (status %d)" % (what, self.lib.gbp_last_error(self.h).decode(), rc))

    def last_error(self):
        """Text of the last error — or of the last recovered incident (a call that returned 0 can leave a `warning: ...` here)."""
        return self.lib.gbp_last_error(self.h).decode()

    # ---- device-resident arrays ----
    # upload / new_keyframe take a dict of torch tensors on the engine's GPU in place of numpy arrays, read / read_priors fill such
    # tensors (out=...) or allocate them (device=True): the library reads and writes them in place, nothing passes through the host
    # and none of these calls waits for the GPU.  The work is ordered on the ctx's stream.  After set_stream(torch.cuda.current_stream()
    # .cuda_stream) that is torch's stream and tensor code before and behind a call is ordered with it as with any torch op; without
    # set_stream the ctx runs on a stream of its own: finish what produces the inputs first (torch.cuda.current_stream().synchronize())
    # and call sync() before touching what a read returned.
    def _sizes(self):
        C_, L, E = self.C, self.L, self.E
        return {"damping": E, "damping_count": E, "mu": 9 * E, "oldmu": 9 * E, "active_flag": E, "robust_flag": E, "cam_scaling": C_, "lmk_scaling": L,
                "cam_weaken_flag": C_, "lmk_weaken_flag": L, "measurements": 2 * E, "meas_variances": E,
                "cam_priors_eta": 6 * C_, "cam_priors_lambda": 36 * C_, "lmk_priors_eta": 3 * L, "lmk_priors_lambda": 9 * L,
                "cam_beliefs_eta": 6 * C_, "cam_beliefs_lambda": 36 * C_, "lmk_beliefs_eta": 3 * L, "lmk_beliefs_lambda": 9 * L}

    @staticmethod
    def _current_device(only_if_initialised=False):
        import sys
        torch = sys.modules.get("torch")
        if only_if_initialised and (torch is None or not torch.cuda.is_initialized()):
            return None      # (torch has not touched the GPU yet: asked again at the first device-tensor call, nothing is initialised for host-array users)
        import torch
        return torch.cuda.current_device()

    def device(self):
        """torch.device of the GPU the ctx was created on (the current device at construction; where torch had not initialised the GPU
        by then: the current device at the first call that needs to know, so do not switch devices in between)"""
        import torch
        if self._device is None:
            self._device = self._current_device()
        return torch.device("cuda", self._device)

    def _device_struct(self, struct, tensors, keep):
        dev = next((a.device for a in tensors.values() if cabi.is_device_tensor(a)), None)
        if dev is None:
            raise TypeError("expected torch tensors on the engine's GPU")
        if dev.type == "cuda":
            dev = self.device()      # (every tensor must be on the ctx's GPU; the C-ABI checks the same from the pointers)
        return cabi.fill_struct_device(struct, tensors, self._sizes(), dev, keep)

    def _device_out(self, fields, device):
        import torch
        dev = self.device() if device is True else torch.device(device)
        sz = self._sizes()
        dt = {cabi.c_f32p: torch.float32, cabi.c_i32p: torch.int32, cabi.c_u32p: torch.int32}
        return {n: torch.empty(sz[n], dtype=dt[t], device=dev) for n, t in fields}

    # ---- program list ----
    def upload(self, state):
        """state: dict of numpy arrays — or of torch tensors on the engine's GPU (read in place, not blocking)."""
        keep = []
        if cabi.any_device_tensor(state):
            s = self._device_struct(cabi.GbpStateIn(), state, keep)
        else:
            s = cabi.fill_struct(cabi.GbpStateIn(), state, keep)
        self._chk(self.lib.gbp_upload(self.h, C.byref(s)), "gbp_upload")

    def linearise(self):
        self._chk(self.lib.gbp_linearise(self.h), "gbp_linearise")

    def iterate(self, n=1):
        self._chk(self.lib.gbp_iterate(self.h, int(n)), "gbp_iterate")

    def prepare(self):
        """Pay the one-off costs of the multi-iteration path now (graph capture, instantiation, upload); runs nothing."""
        self._chk(self.lib.gbp_prepare(self.h), "gbp_prepare")

    def weaken_priors(self):
        self._chk(self.lib.gbp_weaken_priors(self.h), "gbp_weaken_priors")

    def read(self, out=None, device=False):
        """Host arrays by default.  out = dict of torch tensors on the engine's GPU: those are filled (members left out are skipped);
        device=True: the same into tensors freshly allocated on the engine's GPU (flags as int32).  Neither waits for the GPU."""
        if out is not None or device:
            if out is None:
                out = self._device_out(cabi.GbpStateOut._fields_, device)
            keep = []
            s = self._device_struct(cabi.GbpStateOut(), out, keep)
            self._chk(self.lib.gbp_read(self.h, C.byref(s)), "gbp_read")
            return out
        out = {"cam_beliefs_eta": np.zeros(6 * self.C, np.float32),
               "cam_beliefs_lambda": np.zeros(36 * self.C, np.float32),
               "lmk_beliefs_eta": np.zeros(3 * self.L, np.float32),
               "lmk_beliefs_lambda": np.zeros(9 * self.L, np.float32),
               "damping": np.zeros(self.E, np.float32),
               "damping_count": np.zeros(self.E, np.int32),
               "robust_flag": np.zeros(self.E, np.uint32)}
        keep = []
        s = cabi.fill_struct(cabi.GbpStateOut(), out, keep)
        self._chk(self.lib.gbp_read(self.h, C.byref(s)), "gbp_read")
        return out

    def read_priors(self, out=None, device=False):
        """as read(): host arrays by default, device tensors with out=... / device=True"""
        if out is not None or device:
            if out is None:
                out = self._device_out(cabi.GbpPriorsOut._fields_, device)
            keep = []
            s = self._device_struct(cabi.GbpPriorsOut(), out, keep)
            self._chk(self.lib.gbp_read_priors(self.h, C.byref(s)), "gbp_read_priors")
            return out
        out = {"cam_priors_eta": np.zeros(6 * self.C, np.float32),
               "cam_priors_lambda": np.zeros(36 * self.C, np.float32),
               "lmk_priors_eta": np.zeros(3 * self.L, np.float32),
               "lmk_priors_lambda": np.zeros(9 * self.L, np.float32)}
        keep = []
        s = cabi.fill_struct(cabi.GbpPriorsOut(), out, keep)
        self._chk(self.lib.gbp_read_priors(self.h, C.byref(s)), "gbp_read_priors")
        return out

    def new_keyframe(self, upd):
        """upd: dict of numpy arrays — or of torch tensors on the engine's GPU (read in place, not blocking)."""
        keep = []
        if cabi.any_device_tensor(upd):
            s = self._device_struct(cabi.GbpKfUpdate(), upd, keep)
        else:
            s = cabi.fill_struct(cabi.GbpKfUpdate(), upd, keep)
        self._chk(self.lib.gbp_new_keyframe(self.h, C.byref(s)), "gbp_new_keyframe")

    # ---- the solution: what a user wants from a finished run (gbp_poplar_amd/post.py, include/gbp_mi355x_post.h) ----
    def solution(self, measurements=None, active_flag=None, device=False):
        """The beliefs as means, marginal covariances and status words per variable — post.moments(read(device=True)) — and, with
        `measurements` [2E] (and `active_flag` [E], default: every edge active; numpy arrays or tensors on the engine's GPU), the
        reprojection residual and its covariance per edge — post.residuals over the graph's cam_id / lmk_id and K.  Returns one dict:
        cam_mean, cam_cov, lmk_mean, lmk_cov, cam_status, lmk_status (+ residual, reproj_cov); see post.py for shapes and meaning.
        Everything is computed on the GPU from the device-resident read.  Where the ctx runs on the caller's stream (set_stream), the
        read and the readout are queued there and nothing waits; where it runs on a stream of its own, THIS CALL BLOCKS: it calls
        sync() between the read and the readout, which is launched on torch's current stream.  device=False (default): numpy
        arrays, which blocks in either case; device=True: tensors on the engine's GPU, valid for work queued behind the call."""
        import torch
        from . import post
        beliefs = self.read(device=True)
        if self._stream is None:
            self.sync()
        dev = self.device()
        with torch.cuda.device(dev):
            stream = self._stream if self._stream is not None else torch.cuda.current_stream().cuda_stream
            out = post.moments(beliefs, stream=stream)
            if measurements is not None:
                if self._edge_ids is None:
                    ids = [np.ctypeslib.as_array(p, shape=(self.E,)) if self.E else np.zeros(0, np.uint32) for p in (self.problem.cam_id, self.problem.lmk_id)]
                    self._edge_ids = [torch.from_numpy(a.view(np.int32).copy()).to(dev) for a in ids]

                def on_gpu(a, ints):
                    if a is None or cabi.is_device_tensor(a):
                        return a
                    a = np.ascontiguousarray(a, dtype=np.uint32 if ints else np.float32).reshape(-1)
                    t = torch.from_numpy(a.view(np.int32) if ints else a).to(dev)
                    if self._stream is not None:      # (staged on torch's current stream, read on the ctx's)
                        torch.cuda.current_stream().synchronize()
                    return t
                out.update(post.residuals(self._edge_ids[0], self._edge_ids[1], [self.problem.K[i] for i in range(9)], out,
                                          on_gpu(measurements, False), on_gpu(active_flag, True), covs=out, stream=stream))
        if device:
            return out
        torch.cuda.synchronize(dev)
        return {k: (v.cpu().numpy().view(np.uint32) if k.endswith("status") else v.cpu().numpy()) for k, v in out.items()}

    # The metric in device memory.  eval / iterate_eval_each / ba_loop with device=True (or out= a contiguous torch.int64 tensor on the
    # engine's GPU, [7] for eval, [n, 7] for the loops) make the library write its gbp_eval_out records there: the call does not wait, the
    # records are valid for work queued behind it on the ctx's stream (set_stream) or after sync(), and the tensor must stay allocated
    # until the next sync() or blocking call of the engine.  Returned: a dict with the keys of eval(), every value a 1-D tensor that views
    # one column of that buffer (sum_norm, sum_half_sq as float64); pass out= and keep it where the records are wanted whole.
    def _eval_buffer(self, out, shape):
        import torch
        if out is None:
            return torch.empty(shape, dtype=torch.int64, device=self.device())
        return cabi.check_eval_buffer(out, shape, self.device())

    @staticmethod
    def _eval_ptr(buf):
        return C.cast(C.c_void_p(buf.data_ptr()), C.POINTER(cabi.GbpEvalOut))

    def eval(self, device=False, out=None):
        """Host numbers by default; device=True / out=...: the record on the engine's GPU, not blocking (see above)."""
        if device or out is not None:
            buf = self._eval_buffer(out, (7,))
            self._chk(self.lib.gbp_eval(self.h, self._eval_ptr(buf)), "gbp_eval")
            return cabi.eval_buffer_views(buf)
        o = cabi.GbpEvalOut()
        self._chk(self.lib.gbp_eval(self.h, C.byref(o)), "gbp_eval")
        return {k: getattr(o, k) for k, _ in o._fields_}

    def eval_begin(self):
        self._chk(self.lib.gbp_eval_begin(self.h), "gbp_eval_begin")

    def iterate_eval(self, n=1):
        """iterate(n) + eval_begin() in one call (fused into one launch on graphs that run in the persistent kernel)."""
        self._chk(self.lib.gbp_iterate_eval(self.h, int(n)), "gbp_iterate_eval")

    def iterate_eval_each(self, n, device=False, out=None):
        """n iterations with the metric after every one (blocking); one launch per burst on graphs that run in the
        persistent kernel.  Returns a list of n dicts like eval().  device=True / out=...: the n records on the engine's GPU, not
        blocking; returns one dict of length-n tensors."""
        n = int(n)
        if device or out is not None:
            buf = self._eval_buffer(out, (n, 7))
            self._chk(self.lib.gbp_iterate_eval_each(self.h, n, self._eval_ptr(buf) if n else None), "gbp_iterate_eval_each")
            return cabi.eval_buffer_views(buf)
        arr = (cabi.GbpEvalOut * max(n, 1))()
        self._chk(self.lib.gbp_iterate_eval_each(self.h, n, arr), "gbp_iterate_eval_each")
        return [{k: getattr(arr[i], k) for k, _ in arr[i]._fields_} for i in range(n)]

    def ba_loop(self, n, iter0, steps, metrics=True, device=False, out=None):
        """n passes of the body of the reference's loop from loop index iter0 (prior weakening where the loop weakens, the iteration,
        the metric): gbp_ba_loop.  Returns a list of n dicts like eval().  device=True / out=...: the n records on the engine's GPU,
        not blocking; returns one dict of length-n tensors."""
        n = int(n)
        if metrics and (device or out is not None):
            buf = self._eval_buffer(out, (n, 7))
            if n:
                self._chk(self.lib.gbp_ba_loop(self.h, n, int(iter0), int(steps), self._eval_ptr(buf)), "gbp_ba_loop")
            return cabi.eval_buffer_views(buf)
        if not metrics:      # the passes without the metric: not blocking, returns nothing
            self._chk(self.lib.gbp_ba_loop(self.h, n, int(iter0), int(steps), None), "gbp_ba_loop")
            return None
        arr = (cabi.GbpEvalOut * max(n, 1))()
        self._chk(self.lib.gbp_ba_loop(self.h, n, int(iter0), int(steps), arr), "gbp_ba_loop")
        return [{k: getattr(arr[i], k) for k, _ in arr[i]._fields_} for i in range(n)]

    def eval_end(self):
        o = cabi.GbpEvalOut()
        self._chk(self.lib.gbp_eval_end(self.h, C.byref(o)), "gbp_eval_end")
        return {k: getattr(o, k) for k, _ in o._fields_}

    def sync(self):
        self._chk(self.lib.gbp_sync(self.h), "gbp_sync")

    def timing(self, reset=False):
        t = cabi.GbpTimingOut()
        self._chk(self.lib.gbp_timing(self.h, C.byref(t), int(reset)), "gbp_timing")
        return {k: getattr(t, k) for k, _ in t._fields_}

    def set_profiling(self, on):
        self._chk(self.lib.gbp_set_profiling(self.h, int(bool(on))), "gbp_set_profiling")

    # ---- split-phase (sharded) ----
    def set_stream(self, stream_handle):
        self._chk(self.lib.gbp_set_stream(self.h, C.c_void_p(stream_handle)), "gbp_set_stream")
        self._stream = int(stream_handle) if stream_handle else None      # (NULL / 0: back on the ctx's own stream)

    def set_exchange_buffers(self, send_ptr, recv_ptr):
        self._chk(self.lib.gbp_set_exchange_buffers(self.h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr)),
                  "gbp_set_exchange_buffers")

    def iterate_begin(self):
        self._chk(self.lib.gbp_iterate_begin(self.h), "gbp_iterate_begin")

    def iterate_local(self):
        self._chk(self.lib.gbp_iterate_local(self.h), "gbp_iterate_local")

    def iterate_end(self):
        self._chk(self.lib.gbp_iterate_end(self.h), "gbp_iterate_end")

    def refresh_begin(self):
        self._chk(self.lib.gbp_refresh_begin(self.h), "gbp_refresh_begin")

    def refresh_end(self):
        self._chk(self.lib.gbp_refresh_end(self.h), "gbp_refresh_end")

    def linearise_factors(self):
        self._chk(self.lib.gbp_linearise_factors(self.h), "gbp_linearise_factors")

    # ---- library-owned exchange (RCCL from the C++ host) ----
    def comm_unique_id(self):
        """Rank 0: the 128-byte RCCL id every rank passes to comm_init_rccl (distribute it with your launcher's means)."""
        buf = C.create_string_buffer(128)
        rc = self.lib.gbp_comm_unique_id(buf)
        if rc != 0:
            raise GbpError("gbp_comm_unique_id: %s (status %d)" % (self.lib.gbp_last_error(None).decode(), rc))
        return buf.raw

    def comm_init_rccl(self, id128):
        buf = C.create_string_buffer(bytes(id128), 128)
        self._chk(self.lib.gbp_comm_init_rccl(self.h, buf), "gbp_comm_init_rccl")

    def comm_init(self, region_address, transport=0):
        """Collective over the ranks of a launcher-made group: attaches the library's communicator over `transport` (0 auto, 1 rccl,
        2 host-staged, 3 p2p, 4 p2p-slices, 5 measured: the library times what the ranks can form and keeps the fastest — see
        comm_describe()["measured"]).  region_address: the address of the shared region (gbp_comm_region_bytes / gbp_comm_region_init)
        as this process maps it."""
        self._chk(self.lib.gbp_comm_init(self.h, C.c_void_p(int(region_address)), int(transport)), "gbp_comm_init")

    def comm_describe(self):
        """dict: rank, world, device, pci_bus_id, transport, library (resolved path of librccl), library_version, two_streams,
        selected_by ("caller", "rule", "measurement"), after comm_init(..., 5) measured: one dict per candidate, and metric: how the
        loops with the metric (ba_loop, iterate_eval_each) have run on this ctx — path ("riding" in the sharded iterations, "per-pass",
        "none"), passes_riding, passes_per_pass, reason (why the last burst did not ride)"""
        import json
        buf = C.create_string_buffer(16384)
        self._chk(self.lib.gbp_comm_describe(self.h, buf, 16384), "gbp_comm_describe")
        return json.loads(buf.value.decode())

    def comm_set_schedule(self, two_streams):
        self._chk(self.lib.gbp_comm_set_schedule(self.h, int(bool(two_streams))), "gbp_comm_set_schedule")

    def comm_probe(self, reps=50):
        """mean duration (us) of one all-gather of the camera partial buffers, `reps` back to back (collective)"""
        us = C.c_double(0.0)
        self._chk(self.lib.gbp_comm_probe(self.h, int(reps), C.byref(us)), "gbp_comm_probe")
        return us.value

    def comm_transport(self):
        return self.lib.gbp_comm_transport(self.h).decode()

    def graph_state(self):
        """2: bursts run inside the persistent kernel (small graph); 1: gbp_iterate replays a captured hipGraph;
        0: nothing captured yet; -1: capture failed, direct launches."""
        return int(self.lib.gbp_graph_state(self.h))

    def comm_barrier(self):
        self._chk(self.lib.gbp_comm_barrier(self.h), "gbp_comm_barrier")

    def eval_global(self):
        o = cabi.GbpEvalOut()
        self._chk(self.lib.gbp_eval_global(self.h, C.byref(o)), "gbp_eval_global")
        return {k: getattr(o, k) for k, _ in o._fields_}

    # ---- raw state for parity tests ----
    def _need_hooks(self):
        if not self.hooks:
            raise GbpError("internal state is reachable only through the test-hooks build: GbpEngine(..., hooks=True)")

    def _debug(self, what, na, nb):
        self._need_hooks()
        a, b = np.zeros(na, np.float32), np.zeros(nb, np.float32)
        self._chk(self.lib.gbp_debug_get(self.h, what, cabi.ptr(a, cabi.c_f32p), cabi.ptr(b, cabi.c_f32p)),
                  "gbp_debug_get")
        return a, b

    def persist_flow(self, on):
        """bursts without the metric in the persistent kernel: tagged-record hand-offs (default) or counter barriers (A/B, tests)"""
        self._need_hooks()
        self._chk(self.lib.gbp_debug_persist_flow(self.h, int(bool(on))), "gbp_debug_persist_flow")

    def sweep_variant(self):
        """(SweepArgs.policy bits, segment-skipping instantiation?) of the sweep this ctx launches on the two-kernel path (test hook)"""
        self._need_hooks()
        pol, seg = C.c_uint32(0), C.c_int(0)
        self._chk(self.lib.gbp_debug_sweep_variant(self.h, C.byref(pol), C.byref(seg)), "gbp_debug_sweep_variant")
        return int(pol.value), bool(seg.value)

    def persist_verify(self, on):
        """redundant records in the persistent kernel (test hook): every tagged record published twice and compared by its consumers;
        returns the mismatches counted since the last call"""
        self._need_hooks()
        n = C.c_uint64(0)
        self._chk(self.lib.gbp_debug_persist_verify(self.h, int(bool(on)), C.byref(n)), "gbp_debug_persist_verify")
        return int(n.value)

    def persist_counters(self, seq=None, epoch_base=None):
        """(number of the ctx's last launch of the persistent kernel, arrivals its barrier counter has seen) after the call (test hook).
        seq / epoch_base: store these first (one of them alone: the other keeps its value); the ctx is settled before."""
        self._need_hooks()
        get = (C.c_uint32 * 2)()
        if seq is not None or epoch_base is not None:
            self._chk(self.lib.gbp_debug_persist_counters(self.h, None, get), "gbp_debug_persist_counters")
            put = (C.c_uint32 * 2)(get[0] if seq is None else int(seq) & 0xffffffff, get[1] if epoch_base is None else int(epoch_base) & 0xffffffff)
            self._chk(self.lib.gbp_debug_persist_counters(self.h, put, get), "gbp_debug_persist_counters")
        else:
            self._chk(self.lib.gbp_debug_persist_counters(self.h, None, get), "gbp_debug_persist_counters")
        return int(get[0]), int(get[1])

    def factor_potentials(self):
        return self._debug(0, 9 * self.E, 81 * self.E)

    def set_factor_potentials(self, eta, lam):
        self._need_hooks()
        eta, lam = np.ascontiguousarray(eta, np.float32), np.ascontiguousarray(lam, np.float32)
        self._chk(self.lib.gbp_debug_set_factor_potentials(self.h, cabi.ptr(eta, cabi.c_f32p), cabi.ptr(lam, cabi.c_f32p)),
                  "gbp_debug_set_factor_potentials")

    def messages(self):
        ce, cl = self._debug(1, 6 * self.E, 36 * self.E)
        le, ll = self._debug(2, 3 * self.E, 9 * self.E)
        return {"cam_eta": ce, "cam_lambda": cl, "lmk_eta": le, "lmk_lambda": ll}

    def mu(self):
        return self._debug(3, 9 * self.E, self.E)
