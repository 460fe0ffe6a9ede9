"""Host-side engine: turns PyTorch-ROCm tensors into raw pointers for the C ABI.

One instance per process.  It owns no device memory: every buffer (state, E, Vt, ...)
is a torch tensor allocated by the caller's caching allocator on the caller's current
stream, which is also the stream the kernels are enqueued on -- so ordering with the
surrounding PyTorch ops needs no extra synchronisation.
"""
import torch

from . import _lib

NW, SW = _lib.SDP_NW, _lib.SDP_SW


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NULL_CTX = _NullCtx()


def _ptr(t):
    """A tensor's address; None (a null pointer) and integers go as they are."""
    return t.data_ptr() if isinstance(t, torch.Tensor) else t


def check_args(ref, dtype=None, shape=None, contiguous=False, dtype_error=TypeError, **tensors):
    """The C ABI takes raw addresses: refuse every tensor of `tensors` (name=tensor; None is skipped) that is not of `dtype`,
    not on the device of `ref`, not of `shape`, or -- where `contiguous` is asked -- not contiguous.  dtype / shape None:
    any.  Raises `dtype_error` for the dtype, ValueError for the rest."""
    for name, t in tensors.items():
        if t is None:
            continue
        if dtype is not None and t.dtype != dtype:
            raise dtype_error(f"{name} must be {dtype}, got {t.dtype}")
        if t.device != ref.device:
            raise ValueError(f"{name} is on {t.device}, expected {ref.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if contiguous and not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous, got strides {t.stride()}")


def _sweep_dtype(t):
    """The precision a sweep runs in, from its leading tensor (theta, or the state): float64 stays, all else is float32's."""
    return torch.float64 if t.dtype == torch.float64 else torch.float32


EXACT_STATE = 0x100  # include/sdp.h: SDP_EXACT_STATE
ET_BROADCAST = 0x200  # include/sdp.h: SDP_ET_BROADCAST
REF_ROUNDING = 0x400  # include/sdp.h: SDP_REF_ROUNDING
REF = "ref"           # value of `exact_state` that selects it: the state is then the reference's own (B, N, M, 3) fp32
F64 = "f64"           # value of `exact_state` that rides along with float64 tensors: the state is (B, N, M, 3) float64
TRACEBACK_RULES = {"cpu": 0, "cuda": 1}  # include/sdp.h: SDP_TRACEBACK_CPU / SDP_TRACEBACK_CUDA


class HipEngine:
    """Thin veneer over libsdp_hip.so.  All tensors must be fp32 (the four sweeps: or float64), on one ROCm device.
    Every launch goes through call(); every argument check through check_args()."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        # optional profiling hook (bench.py): callable(name) -> context manager that brackets one
        # kernel launch on the current stream, e.g. with a pair of events.  None = no overhead.
        self.launch_hook = None
        # per-pass wave-count override for experiments and tests ({0 fwd, 1 bwd, 2 adj-fwd, 3 adj-bwd, 4 value-only fwd} -> waves);
        # travels with each call as SDP_WAVES(w), the library keeps no tuning state
        self.force_waves = {}
        # measurement control (bench.py's `no_skip` figures): False = the backward sweep runs every chunk (SDP_NO_ZERO_SKIP);
        # results are bit-identical either way
        self.zero_skip = True
        self._labels = {}

    def _label(self, pass_, B, N, M, has_lens, exact, dev, default):
        """Name of the kernel a launch will use (for the launch hook: bench.py's per-kernel timers must carry the names the
        rocprofv3 summaries carry).  Asked of the library's own launch policy (sdp_plan, sdp_kernel_name), once per problem."""
        if self.launch_hook is None:
            return default
        key = (pass_, B, N, M, bool(has_lens), bool(exact), dev)
        got = self._labels.get(key)
        if got is None:
            import ctypes
            kid = ctypes.c_int(-1)
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            rc = self.lib.sdp_plan(pass_, B, N, M, 1 if has_lens else 0, 1 if exact else 0, cus, ctypes.byref(kid), None, None, None)
            name = self.lib.sdp_kernel_name(kid.value) if rc == 0 else None
            got = name.decode() if name else default
            self._labels[key] = got
        return got

    def _v(self, pass_, variant):
        w = self.force_waves.get(pass_, 0)
        return variant | (_lib.SDP_WAVES(w) if w else 0)

    def check_device(self, device=None):
        """Raise HandoffTimeout if a kernel launched earlier on `device` reported a strip hand-off that timed out.
        Host-side read: synchronise first to cover work that is still in flight."""
        import ctypes
        dev = torch.cuda.current_device() if device is None else device
        info = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.sdp_device_status(dev, info), "sdp_device_status")
        return list(info)

    def call(self, entry, label, dev, *args):
        """The one way from Python to a launching entry of the C ABI: `entry`(*args, dev, stream) with device `dev` current
        and on its current stream, bracketed by the launch hook under `label`.  Tensors go as their addresses, None as a
        null pointer, integers as they are; a status other than 0 raises under the name of `entry` (_lib.check)."""
        args = [_ptr(a) for a in args]
        with torch.cuda.device(dev), (self.launch_hook(label) if self.launch_hook is not None else _NULL_CTX):
            rc = getattr(self.lib, entry)(*args, dev, self._stream(dev))
        _lib.check(rc, entry)

    # ---- helpers -------------------------------------------------------------------
    @staticmethod
    def device_of(t):
        """Index of the ROCm device `t` lives on -- the launch device of a call."""
        if not t.is_cuda:
            raise RuntimeError(
                "deepblast_amd runs on a ROCm device only (got a CPU tensor); there is no CPU fallback. "
                "Move theta/A to 'cuda'.")
        return t.device.index if t.device.index is not None else torch.cuda.current_device()

    @staticmethod
    def _stream(dev):
        return torch.cuda.current_stream(dev).cuda_stream

    def max_cols(self):
        return self.lib.sdp_max_cols()

    def scores_backward_ws_bytes(self, B, N, M):
        return self.lib.sdp_scores_backward_ws_bytes(B, N, M)

    def new_state(self, B, N, M, device, derivative=False, ref=False):
        """Opaque buffer for Q (packed: two 20-bit weights, 5 bytes per cell) or, with derivative=True, for Qd (float2 per cell); ref: the
        reference-rounding mode's (B, N, M, 3) fp32 for either."""
        if ref:
            nbytes = self.lib.sdp_state_bytes_v(B, N, M, REF_ROUNDING)
        else:
            nbytes = (self.lib.sdp_state_d_bytes if derivative else self.lib.sdp_state_bytes)(B, N, M)
        return torch.empty(nbytes // 4, dtype=torch.float32, device=device)

    @staticmethod
    def _state_flags(exact_state):
        """`exact_state` of forward / backward -> flag bits: False = packed, True = float2, "ref" = reference rounding."""
        if isinstance(exact_state, str):
            if exact_state != REF:
                raise ValueError(f"exact_state must be False, True or {REF!r}, got {exact_state!r}")
            return REF_ROUNDING
        return EXACT_STATE if exact_state else 0

    @staticmethod
    def _lens(lens, B, device):
        if lens is None:
            return None
        lens = torch.as_tensor(lens, dtype=torch.int32, device=device).contiguous()
        if lens.shape != (B, 2):
            raise ValueError(f"lengths must have shape ({B}, 2), got {tuple(lens.shape)}")
        return lens

    def _sweep(self, pass_, dtype, variant, fast_flags=0, plan=None):
        """-> (entry, label, variant word) of sweep `pass_` (0 fwd, 1 bwd, 2 adj-fwd, 3 adj-bwd) on tensors of `dtype`.
        float32: the forced wave count and `fast_flags` join `variant`; plan = (B, N, M, has_lens, exact, dev) asks the
        library which build it will launch (the label).  float64: the entries take the bare `variant`."""
        suffix, labels, _ = _PRECISIONS[dtype]
        label = labels[pass_]
        if dtype == torch.float32:
            variant = self._v(pass_, variant) | fast_flags
            if plan is not None:
                label = self._label(pass_, *plan, label)
        return _SWEEPS[pass_] + suffix, label, variant

    # ---- the four passes -----------------------------------------------------------
    # float64 tensors (include/sdp.h: sdp_*_f64) take the same four methods.  The reference's CPU classes take float64 as it
    # comes (its tests: decoding, gradcheck, gradgradcheck on .double() tensors, deepblast/tests/test_nw.py:46-90).  Here: the
    # reference-arithmetic kernels with float64 storage, one workgroup per pair -- for tests and small problems, not a second
    # fast path.  The state is the reference's own (B, N, M, 3) weights in float64, and the other three sweeps recognise it by
    # its dtype; there is no pair_range / out, and none of the fast path's variant bits (_PRECISIONS, _sweep).
    def forward(self, theta, A, variant, lens=None, exact_state=False):
        """-> (Vt (B,), state).  Replaces _forward_pass_kernel (nw_cuda.py:74-79).

        exact_state=False: the compact state the backward sweep reads; True: Q as float2, which the two
        adjoint sweeps need (include/sdp.h, SDP_EXACT_STATE); "ref": the reference's arithmetic and its own
        (B,N,M,3) fp32 Q (SDP_REF_ROUNDING) -- the other three sweeps must then be asked for the same."""
        dev = self.device_of(theta)
        dtype = _sweep_dtype(theta)
        check_args(theta, dtype, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        fast = dtype == torch.float32
        state = _PRECISIONS[dtype][2](self, B, N, M, theta.device, derivative=bool(exact_state), ref=exact_state == REF)
        Vt = torch.empty(B, dtype=dtype, device=theta.device)
        # (the general-pitch builds are chosen from the pointers' alignment inside the library: the label then names the aligned twin)
        entry, label, v = self._sweep(0, dtype, variant, self._state_flags(exact_state) if fast else 0,
                                      (B, N, M, lens is not None, exact_state is True, dev))
        self.call(entry, label, dev, theta, A, state, Vt, B, N, M, lens, v)
        return Vt, state

    def forward_value(self, theta, A, variant, lens=None):
        """-> Vt (B,) and nothing else: the forward sweep for callers that never differentiate (scoring / search; the
        reference's NeuralAligner.score, alignment.py:127-137).  No state is formed or allocated (include/sdp.h:
        sdp_forward_value_f32) -- only Vt and, with lengths, a workspace of a few KB.  float64 tensors take the float64
        forward (a test path) and drop its state."""
        dev = self.device_of(theta)
        if theta.dtype == torch.float64:
            return self.forward(theta, A, variant, lens)[0]
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        ws = None
        if lens is not None:
            ws = torch.empty(max(self.lib.sdp_forward_value_ws_bytes(B, N, M), 4) // 4, dtype=torch.int32, device=theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_forward_value_f32", self._label(4, B, N, M, lens is not None, False, dev, "sdp_val_kernel"), dev,
                  theta, A, Vt, ws, B, N, M, lens, self._v(4, variant))
        return Vt

    def state_pair_bytes(self, N, M, exact_state=False):
        """Bytes between the records of consecutive pairs in the state buffer (include/sdp.h: sdp_state_pair_stride)."""
        return self.lib.sdp_state_pair_stride(N, M, 1 if exact_state else 0)

    def backward(self, Et, state, shape, variant, lens=None, exact_state=False, pair_range=None, out=None, no_fill=False):
        """-> E (B,N,M).  Replaces _backward_pass_kernel (nw_cuda.py:98-102).

        exact_state: `state` came from forward(..., exact_state=True).
        pair_range=(lo, hi), out=(B,N,M) tensor: sweep only pairs lo..hi-1 of the batch, writing out[lo:hi] (the
        other rows of `out` are not touched) -- the backward sweep of a batch in pieces, so that a collective on
        piece k can run under the sweep of piece k+1 (distributed.py).  Needs lens=None.  The library finds the
        pairs' records in `state` itself (sdp_backward_range_f32 takes the whole batch's buffers and the range).
        no_fill (with lens): E outside each pair's block is NOT written (SDP_NO_FILL) -- for consumers that mask by the
        same lengths and never read it; the default zero-fills, as the public contract says."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, Et=Et)
        dtype = _sweep_dtype(state)
        fast = dtype == torch.float32
        if not fast and (pair_range is not None or out is not None):
            raise ValueError("the float64 path sweeps whole batches (no pair_range / out)")
        Et, bcast = self._et(Et, B, dtype)
        lens = self._lens(lens, B, state.device)
        if out is None:
            out = torch.empty((B, N, M), dtype=dtype, device=state.device)
        else:
            check_args(state, torch.float32, (B, N, M), True, ValueError, out=out)
        flags = 0
        if fast:
            flags = self._state_flags(exact_state) | (0 if self.zero_skip else _lib.SDP_NO_ZERO_SKIP)
            flags |= _lib.SDP_NO_FILL if (no_fill and lens is not None) else 0
        entry, label, v = self._sweep(1, dtype, variant | (ET_BROADCAST if bcast else 0), flags,
                                      (B, N, M, lens is not None, exact_state is True, dev))
        if pair_range is None:
            self.call(entry, label, dev, Et, state, out, B, N, M, lens, v)
        else:
            lo, hi = pair_range
            if lens is not None:
                raise ValueError("pair_range needs lens=None")
            if not (0 <= lo < hi <= B):
                raise ValueError(f"pair_range {pair_range} outside the batch of {B}")
            self.call("sdp_backward_range_f32", label, dev, Et, state, out, B, N, M, lo, hi - lo, v)
        return out

    @staticmethod
    def _et(Et, B, dtype):
        """-> (tensor whose data_ptr the kernel reads, broadcast flag).  The usual (B,) fp32 contiguous cotangent goes as
        it is.  A broadcast scalar -- what `Vt.sum().backward()` hands over: a stride-0 expand of one element -- goes as
        that one element with SDP_ET_BROADCAST instead of being expanded into B floats by a kernel of its own.
        float64: only a one-element Et is broadcast."""
        if dtype == torch.float64:
            Et = Et.to(dtype)
            return (Et, True) if Et.numel() == 1 else (Et.expand(B).contiguous(), False)
        if Et.dtype == torch.float32 and Et.dim() <= 1:
            if Et.numel() == 1 or (Et.shape == (B,) and Et.stride(0) == 0):
                return Et, True
            if Et.shape == (B,) and Et.is_contiguous():
                return Et, False
        return Et.to(torch.float32).expand(B).contiguous(), False

    def adjoint_forward(self, state, Ztheta, ZA, variant, lens=None, ref=False):
        """-> (Vtd (B,), state_d).  Replaces _adjoint_forward_pass_kernel (nw_cuda.py:134-139).
        ref: `state` came from forward(..., exact_state="ref"); the Hessian product is rounded as numpy rounds it."""
        dev = self.device_of(state)
        check_args(state, Ztheta=Ztheta, ZA=ZA)
        dtype = _sweep_dtype(state)
        Ztheta = Ztheta.to(dtype).contiguous()
        B, N, M = Ztheta.shape
        if ZA is not None:
            ZA = ZA.to(dtype).contiguous()
        lens = self._lens(lens, B, state.device)
        state_d = _PRECISIONS[dtype][2](self, B, N, M, state.device, derivative=True, ref=ref)
        Vtd = torch.empty(B, dtype=dtype, device=state.device)
        entry, label, v = self._sweep(2, dtype, variant, REF_ROUNDING if ref else 0)
        self.call(entry, label, dev, state, Ztheta, ZA, Vtd, state_d, B, N, M, lens, v)
        return Vtd, state_d

    def adjoint_forward_loss(self, state, ref, pred, G, scale, kind, variant, lens=None):
        """Adjoint forward sweep seeded with scale[b] * d(loss term)/d(pred) formed in the kernel (include/sdp.h:
        sdp_adjoint_forward_loss_f32).  -> (Vtd (B,), state_d)."""
        dev = self.device_of(state)
        check_args(state, torch.float32, first=ref, pred=pred, G=G, scale=scale)
        ref, pred, G, scale = ref.contiguous(), pred.contiguous(), G.contiguous(), scale.contiguous()
        B, N, M = pred.shape
        lens = self._lens(lens, B, state.device)
        state_d = self.new_state(B, N, M, state.device, derivative=True)
        Vtd = torch.empty(B, dtype=torch.float32, device=state.device)
        self.call("sdp_adjoint_forward_loss_f32", "sdp_adj_fwd_kernel", dev, state, ref, pred, G, scale, kind, Vtd, state_d,
                  B, N, M, lens, self._v(2, variant))
        return Vtd, state_d

    def adjoint_backward(self, E, state, state_d, variant, lens=None, ref=False):
        """-> Ed (B,N,M).  Replaces _adjoint_backward_pass_kernel (nw_cuda.py:160-165).  ref: as for adjoint_forward."""
        dev = self.device_of(state)
        dtype = _sweep_dtype(state)
        check_args(state, dtype, E=E, state_d=state_d)
        E = E.contiguous()
        B, N, M = E.shape
        lens = self._lens(lens, B, state.device)
        Ed = torch.empty((B, N, M), dtype=dtype, device=state.device)
        entry, label, v = self._sweep(3, dtype, variant, (REF_ROUNDING if ref else 0) | (0 if self.zero_skip else _lib.SDP_NO_ZERO_SKIP))
        self.call(entry, label, dev, E, state, state_d, Ed, B, N, M, lens, v)
        return Ed

    # ---- the true gap-score gradient (include/sdp.h: sdp_gap_gradient*) -----------------------
    def gap_gradient(self, E, state, shape, variant, lens=None, exact_state=False, no_fill=False):
        """-> G (B,N,M) = E * (Qx + Qy) = Et . dVt/dA, from the E of backward() and the state it read.  exact_state, lens,
        no_fill: what backward() was given (no_fill: G outside each pair's block is not written either)."""
        dev = self.device_of(state)
        B, N, M = shape
        dtype = _sweep_dtype(state)
        check_args(state, dtype, (B, N, M), E=E)
        E = E.contiguous()
        lens = self._lens(lens, B, state.device)
        G = torch.empty((B, N, M), dtype=dtype, device=state.device)
        if dtype == torch.float64:
            self.call("sdp_gap_gradient_f64", "sdp_gap_rows_f64_kernel", dev, E, state, G, B, N, M, lens, variant)
        else:
            flags = self._state_flags(exact_state) | (_lib.SDP_NO_FILL if (no_fill and lens is not None) else 0)
            self.call("sdp_gap_gradient_f32", "sdp_gap_rows_kernel" if exact_state == REF else "sdp_gap_kernel", dev,
                      E, state, G, B, N, M, lens, variant | flags)
        return G

    def gap_gradient2(self, E, Ed, state, state_d, variant, lens=None, ref=False):
        """-> Gd (B,N,M) = Ed * (Qx + Qy) + E * (Qdx + Qdy), from the inputs and results of the adjoint pair run with ZA = ZG:
        the gradient of <Ztheta, E> + <ZG, G> with respect to A.  Zero outside each pair's block.  ref: as for adjoint_forward."""
        dev = self.device_of(state)
        dtype = _sweep_dtype(state)
        B, N, M = E.shape
        check_args(state, dtype, (B, N, M), E=E, Ed=Ed)
        check_args(state, dtype, state_d=state_d)
        E, Ed = E.contiguous(), Ed.contiguous()
        lens = self._lens(lens, B, state.device)
        Gd = torch.empty((B, N, M), dtype=dtype, device=state.device)
        if dtype == torch.float64:
            self.call("sdp_gap_gradient2_f64", "sdp_gap2_rows_f64_kernel", dev, E, Ed, state, state_d, Gd, B, N, M, lens, variant)
        else:
            self.call("sdp_gap_gradient2_f32", "sdp_gap2_rows_kernel" if ref else "sdp_gap2_kernel", dev,
                      E, Ed, state, state_d, Gd, B, N, M, lens, variant | (REF_ROUNDING if ref else 0))
        return Gd

    def traceback(self, grad, lens=None, rule="cpu"):
        """Batched traceback on the device -> (states (B,cap,3) int32, counts (B,) int32).

        rule: "cpu" = the CPU classes' walk (nw.py:401-444), "cuda" = the walk of the GPU classes this library
        replaces (nw_cuda.py:273-317: stops as soon as one neighbour is off the matrix)."""
        if rule not in TRACEBACK_RULES:
            raise ValueError(f"traceback rule must be one of {sorted(TRACEBACK_RULES)}, got {rule!r}")
        dev = self.device_of(grad)
        grad = grad.detach().to(torch.float32).contiguous()
        B, N, M = grad.shape
        lens = self._lens(lens, B, grad.device)
        cap = self.lib.sdp_traceback_capacity(N, M)
        states = torch.empty((B, cap, 3), dtype=torch.int32, device=grad.device)
        counts = torch.empty(B, dtype=torch.int32, device=grad.device)
        self.call("sdp_traceback_rule_i32", "sdp_traceback_kernel", dev, grad, states, counts, B, N, M, lens, TRACEBACK_RULES[rule])
        return states, counts

    # ---- the hard-max operator (include/sdp.h: sdp_hard_*) -------------------------------
    def _hard_variant(self, variant, ymx, waves=True):
        """`variant` of the sdp_hard_* entries; waves=False for the walk, which runs one wave per pair and takes no SDP_WAVES."""
        w = self.force_waves.get("hard", 0) if waves else 0
        return variant | (_lib.SDP_HARD_TIES_YMX if ymx else 0) | (_lib.SDP_WAVES(w) if w else 0)

    def hard_forward(self, theta, A, variant, lens=None, ymx=False):
        """-> (Vt (B,), state): the max-plus sweep and its 2-bit pointers (opaque int32 tensor of sdp_hard_state_bytes).
        ymx: theta and A are a TRANSPOSED problem -- ties are scanned so that the path is the untransposed sweep's."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nbytes = self.lib.sdp_hard_state_bytes(B, N, M)
        state = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_hard_forward_f32", "sdp_hard_fwd_kernel", dev, theta, A, state, Vt, B, N, M, lens, self._hard_variant(variant, ymx))
        return Vt, state

    def hard_forward_value(self, theta, A, variant, lens=None, ymx=False):
        """-> Vt (B,) alone: the same sweep with the pointers compiled out (the same bits)."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_hard_forward_value_f32", "sdp_hard_val_kernel", dev, theta, A, Vt, B, N, M, lens, self._hard_variant(variant, ymx))
        return Vt

    def hard_walk(self, state, shape, variant, lens=None, Et=None, ymx=False, want_E=True, want_states=True, E_out=None,
                  states_out=None):
        """The walk along the pointers of hard_forward -> (E (B,N,M) or None, states (B,cap,3) int32 or None, counts (B,) or None).
        E: Et[b] on pair b's path, +0 on every other cell of its plane (always written in full); states / counts: the path
        and its padding in traceback()'s format.  E_out / states_out: buffers to write into instead of fresh ones."""
        dev = self.device_of(state)
        B, N, M = shape
        lens = self._lens(lens, B, state.device)
        E = states = counts = None
        if want_E:
            if Et is None:
                raise ValueError("hard_walk: E needs Et")
            check_args(state, Et=Et)
            Et = Et.detach().to(torch.float32).expand(B).contiguous()
            check_args(state, torch.float32, (B, N, M), True, ValueError, E_out=E_out)
            E = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if E_out is None else E_out
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            check_args(state, torch.int32, (B, cap, 3), True, ValueError, states_out=states_out)
            states = torch.empty((B, cap, 3), dtype=torch.int32, device=state.device) if states_out is None else states_out
            counts = torch.empty(B, dtype=torch.int32, device=state.device)
        self.call("sdp_hard_walk_f32", "sdp_hard_walk_kernel", dev, state, Et if want_E else None, E, states, counts, B, N, M, lens,
                  self._hard_variant(variant, ymx, waves=False))
        return E, states, counts

    # ---- local alignment on the hard-max family (include/sdp.h: sdp_hard_local_*) ----------
    def hard_local_forward(self, theta, A, variant, lens=None, ymx=False):
        """-> (Vt (B,), state, ends (B, 2) int32): the max-plus sweep with the zero floor -- Vt the best cell, ends its 0-based
        (i, j), (-1, -1) where no cell is positive -- and its 2-bit pointers (code 3: an alignment starts after this cell).
        ymx: theta and A are a TRANSPOSED problem; ends come back in the coordinates handed over."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nbytes = self.lib.sdp_hard_state_bytes(B, N, M)
        state = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        ends = torch.empty((B, 2), dtype=torch.int32, device=theta.device)
        self.call("sdp_hard_local_forward_f32", HARD_LOCAL_KERNELS[111 if ymx else 110], dev, theta, A, state, Vt, ends, B, N, M, lens,
                  self._hard_variant(variant, ymx))
        return Vt, state, ends

    def hard_local_forward_value(self, theta, A, variant, lens=None, ymx=False, want_ends=True):
        """-> (Vt (B,), ends (B, 2) int32 or None): the same sweep with the pointers compiled out (the same bits)."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        ends = torch.empty((B, 2), dtype=torch.int32, device=theta.device) if want_ends else None
        self.call("sdp_hard_local_forward_value_f32", HARD_LOCAL_KERNELS[113 if ymx else 112], dev, theta, A, Vt, ends, B, N, M, lens,
                  self._hard_variant(variant, ymx))
        return Vt, ends

    def hard_local_walk(self, state, ends, shape, variant, lens=None, Et=None, ymx=False, want_E=True, want_states=True, E_out=None,
                        states_out=None):
        """The walk along the pointers of hard_local_forward, from `ends` -> (E (B,N,M) or None, states (B,cap,3) int32 or None,
        counts (B,) or None).  E: Et[b] on pair b's path, +0 on every other cell of its plane; states / counts: the path alone
        (no padding), start first; row cap - 1 of states: (number of path cells, i and j of its first cell) -- the alignment's
        start offsets.  E_out / states_out: buffers to write into instead of fresh ones."""
        dev = self.device_of(state)
        B, N, M = shape
        lens = self._lens(lens, B, state.device)
        check_args(state, torch.int32, (B, 2), True, ValueError, ends=ends)
        E = states = counts = None
        if want_E:
            if Et is None:
                raise ValueError("hard_local_walk: E needs Et")
            check_args(state, Et=Et)
            Et = Et.detach().to(torch.float32).expand(B).contiguous()
            check_args(state, torch.float32, (B, N, M), True, ValueError, E_out=E_out)
            E = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if E_out is None else E_out
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            check_args(state, torch.int32, (B, cap, 3), True, ValueError, states_out=states_out)
            states = torch.empty((B, cap, 3), dtype=torch.int32, device=state.device) if states_out is None else states_out
            counts = torch.empty(B, dtype=torch.int32, device=state.device)
        self.call("sdp_hard_local_walk_f32", HARD_LOCAL_KERNELS[114], dev, state, ends, Et if want_E else None, E, states, counts,
                  B, N, M, lens, self._hard_variant(variant, ymx, waves=False))
        return E, states, counts

    # ---- the soft local operator (include/sdp.h: sdp_soft_local_*) ---------------------------
    def soft_local_forward(self, theta, A, lens=None, state_out=None):
        """-> (Vt (B,), state): the soft local sweep and its 16-byte records (opaque float32 tensor of
        sdp_soft_local_state_bytes).  state_out: a buffer of that size to write into instead of a fresh one."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nfloats = max(self.lib.sdp_soft_local_state_bytes(B, N, M), 4) // 4
        check_args(theta, torch.float32, (nfloats,), True, ValueError, state_out=state_out)
        state = torch.empty(nfloats, dtype=torch.float32, device=theta.device) if state_out is None else state_out
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_soft_local_forward_f32", SOFT_LOCAL_KERNELS[130], dev, theta, A, state, Vt, B, N, M, lens, 0)
        return Vt, state

    def soft_local_forward_value(self, theta, A, lens=None):
        """-> Vt (B,) alone: the same sweep with the records compiled out (the same bits); nothing else is allocated."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_soft_local_forward_value_f32", SOFT_LOCAL_KERNELS[131], dev, theta, A, Vt, B, N, M, lens, 0)
        return Vt

    def soft_local_backward(self, state, Vt, Et, shape, lens=None, want_G=True):
        """The mirror sweep over the records of soft_local_forward -> (E (B,N,M), G (B,N,M) or None): Et . dVt/dtheta and
        Et . dVt/dA, +0 outside each pair's block.  Vt: what soft_local_forward returned with `state`."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        E = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        G = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_G else None
        self.call("sdp_soft_local_backward_f32", SOFT_LOCAL_KERNELS[132], dev, state, Vt, Et, E, G, B, N, M, lens, 0)
        return E, G

    def soft_local_adjoint_forward(self, state, Vt, ZE, ZG, shape, lens=None, state_d_out=None):
        """The adjoint forward sweep over the records of soft_local_forward -> (Vtd (B,), state_d): ZE, ZG (B,N,M) the cotangents
        of E and G, one of them may be None (zeros); state_d the dot records (opaque float32 tensor of
        sdp_soft_local_adjoint_state_bytes; state_d_out: a buffer of that size to write into instead of a fresh one)."""
        dev = self.device_of(state)
        B, N, M = shape
        if ZE is None and ZG is None:
            raise ValueError("soft_local_adjoint_forward: ZE and ZG are both None")
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, torch.float32, (B, N, M), ZE=ZE, ZG=ZG)
        ZE, ZG = (None if z is None else z.detach().contiguous() for z in (ZE, ZG))
        lens = self._lens(lens, B, state.device)
        nfloats = max(self.lib.sdp_soft_local_adjoint_state_bytes(B, N, M), 4) // 4
        check_args(state, torch.float32, (nfloats,), True, ValueError, state_d_out=state_d_out)
        state_d = torch.empty(nfloats, dtype=torch.float32, device=state.device) if state_d_out is None else state_d_out
        Vtd = torch.empty(B, dtype=torch.float32, device=state.device)
        self.call("sdp_soft_local_adjoint_forward_f32", SOFT_LOCAL_ADJOINT_KERNELS[140], dev, state, Vt, ZE, ZG, state_d, Vtd, B, N, M,
                  lens, 0)
        return Vtd, state_d

    def soft_local_adjoint_backward(self, state, state_d, Vt, Vtd, Et, shape, lens=None, want_G=True):
        """The adjoint mirror sweep -> (Ed (B,N,M), Gd (B,N,M) or None): the gradients of <ZE,E> + <ZG,G> with respect to theta and
        A, +0 outside each pair's block.  state, Vt: of soft_local_forward; state_d, Vtd: of soft_local_adjoint_forward; Et: what
        soft_local_backward was given."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt, Vtd=Vtd)
        check_args(state, torch.float32, None, True, state_d=state_d)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        Ed = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        Gd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_G else None
        self.call("sdp_soft_local_adjoint_backward_f32", SOFT_LOCAL_ADJOINT_KERNELS[141], dev, state, state_d, Vt, Vtd, Et, Ed, Gd,
                  B, N, M, lens, 0)
        return Ed, Gd

    # ---- alignments sampled from its posterior (include/sdp.h: sdp_soft_local_end_tables_f32, sdp_soft_local_sample_paths_f32) ----
    def soft_local_end_tables(self, state, Vt, shape, lens=None, cdf_out=None, rows_out=None):
        """The end-cell tables over the records of soft_local_forward -> (cdf (B,N,M), rows (B,N+1)) fp32: the running sums of
        w = exp(V - Vt) along every row, and of the rows' totals from exp(-Vt) on.  Only entries inside a pair's block are
        written; fresh tensors are zero outside.  cdf_out / rows_out: buffers to write into instead of fresh ones."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, torch.float32, (B, N, M), True, ValueError, cdf_out=cdf_out)
        check_args(state, torch.float32, (B, N + 1), True, ValueError, rows_out=rows_out)
        lens = self._lens(lens, B, state.device)
        new = torch.empty if lens is None else torch.zeros      # (without lengths every entry is written)
        cdf = new((B, N, M), dtype=torch.float32, device=state.device) if cdf_out is None else cdf_out
        rows = new((B, N + 1), dtype=torch.float32, device=state.device) if rows_out is None else rows_out
        self.call("sdp_soft_local_end_tables_f32", SOFT_LOCAL_SAMPLE_KERNELS[134], dev, state, Vt, cdf, rows, B, N, M, lens, 0)
        return cdf, rows

    def soft_local_sample_paths(self, state, cdf, rows, shape, K, lens=None, seed=0, sample0=0, want_states=True, want_visits=False,
                                want_ends=False):
        """K local alignments per pair drawn from the posterior, on the `state` of soft_local_forward and the tables of
        soft_local_end_tables -> (states (B,K,cap,3) int32 or None, counts (B,K) int32 or None, visits (B,N,M) int32 or None,
        ends (B,K,2) int32 or None).  Sample (b, k) is sample number sample0 + k of pair b under `seed` whatever K is; its list
        -- the path alone, start first -- is RIGHT-aligned in states[b, k]: rows cap-1-counts[b,k] .. cap-2, and row cap-1 holds
        (number of path cells, i, j of the first one), (0, -1, -1) for an empty sample; rows in front of the list are
        unspecified.  ends: the end cell, (-1, -1) for an empty sample.  visits: how many of the K paths pass through each cell."""
        dev = self.device_of(state)
        B, N, M = shape
        if not (want_states or want_visits or want_ends):
            raise ValueError("soft_local_sample_paths: nothing asked for (want_states, want_visits, want_ends)")
        check_args(state, torch.float32, (B, N, M), True, ValueError, cdf=cdf)
        check_args(state, torch.float32, (B, N + 1), True, ValueError, rows=rows)
        lens = self._lens(lens, B, state.device)
        states = counts = visits = ends = None
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            states = torch.empty((B, int(K), cap, 3), dtype=torch.int32, device=state.device)
            counts = torch.empty((B, int(K)), dtype=torch.int32, device=state.device)
        if want_visits:
            visits = torch.zeros((B, N, M), dtype=torch.int32, device=state.device)
        if want_ends:
            ends = torch.empty((B, int(K), 2), dtype=torch.int32, device=state.device)
        self.call("sdp_soft_local_sample_paths_f32", SOFT_LOCAL_SAMPLE_KERNELS[135], dev, state, cdf, rows, states, counts, visits, ends,
                  B, N, M, int(K), int(sample0), int(seed) & 0xffffffffffffffff, lens, 0)
        return states, counts, visits, ends

    # ---- the sparsemax operator (include/sdp.h: sdp_sparsemax_*) ------------------------------
    def _sparsemax_variant(self, variant):
        w = self.force_waves.get("sparsemax", 0)
        return variant | (_lib.SDP_WAVES(w) if w else 0)

    def sparsemax_forward(self, theta, A, variant, lens=None, state_out=None):
        """-> (Vt (B,), state): the sparsemax sweep and its 16-byte records {q_x, q_m, q_y, V} (opaque float32 tensor of
        sdp_sparsemax_state_bytes).  state_out: a buffer of that size to write into instead of a fresh one."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nfloats = max(self.lib.sdp_sparsemax_state_bytes(B, N, M), 4) // 4
        check_args(theta, torch.float32, (nfloats,), True, ValueError, state_out=state_out)
        state = torch.empty(nfloats, dtype=torch.float32, device=theta.device) if state_out is None else state_out
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_sparsemax_forward_f32", SPARSEMAX_KERNELS[150], dev, theta, A, state, Vt, B, N, M, lens,
                  self._sparsemax_variant(variant))
        return Vt, state

    def sparsemax_forward_value(self, theta, A, variant, lens=None):
        """-> Vt (B,) alone: the same sweep with the records compiled out (the same bits); nothing else is allocated."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, A=A)
        theta, A = theta.contiguous(), A.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_sparsemax_forward_value_f32", SPARSEMAX_KERNELS[151], dev, theta, A, Vt, B, N, M, lens,
                  self._sparsemax_variant(variant))
        return Vt

    def sparsemax_backward(self, state, Vt, Et, shape, variant, lens=None, want_G=True):
        """The mirror sweep over the records of sparsemax_forward -> (E (B,N,M), G (B,N,M) or None): Et . dVt/dtheta and
        Et . dVt/dA, +0 outside each pair's block (and below lo for SW).  Vt: what sparsemax_forward returned with `state`."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        E = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        G = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_G else None
        self.call("sdp_sparsemax_backward_f32", SPARSEMAX_KERNELS[152], dev, state, Vt, Et, E, G, B, N, M, lens,
                  self._sparsemax_variant(variant))
        return E, G

    def sparsemax_adjoint_forward(self, state, ZE, ZG, shape, variant, lens=None, state_d_out=None):
        """The adjoint forward sweep over the records of sparsemax_forward -> (Vtd (B,), state_d): ZE, ZG (B,N,M) the cotangents
        of E and G, one of them may be None (zeros); state_d the dot records (opaque float32 tensor of
        sdp_sparsemax_adjoint_state_bytes; state_d_out: a buffer of that size to write into instead of a fresh one)."""
        dev = self.device_of(state)
        B, N, M = shape
        if ZE is None and ZG is None:
            raise ValueError("sparsemax_adjoint_forward: ZE and ZG are both None")
        check_args(state, torch.float32, (B, N, M), ZE=ZE, ZG=ZG)
        ZE, ZG = (None if z is None else z.detach().contiguous() for z in (ZE, ZG))
        lens = self._lens(lens, B, state.device)
        nfloats = max(self.lib.sdp_sparsemax_adjoint_state_bytes(B, N, M), 4) // 4
        check_args(state, torch.float32, (nfloats,), True, ValueError, state_d_out=state_d_out)
        state_d = torch.empty(nfloats, dtype=torch.float32, device=state.device) if state_d_out is None else state_d_out
        Vtd = torch.empty(B, dtype=torch.float32, device=state.device)
        self.call("sdp_sparsemax_adjoint_forward_f32", SPARSEMAX_ADJOINT_KERNELS[154], dev, state, ZE, ZG, state_d, Vtd, B, N, M, lens,
                  self._sparsemax_variant(variant))
        return Vtd, state_d

    def sparsemax_adjoint_backward(self, state, state_d, Et, shape, variant, lens=None, want_G=True):
        """The adjoint mirror sweep -> (Ed (B,N,M), Gd (B,N,M) or None): the gradients of <ZE,E> + <ZG,G> with respect to theta and
        A, +0 outside each pair's block (and below lo for SW).  state: of sparsemax_forward; state_d: of sparsemax_adjoint_forward;
        Et: what sparsemax_backward was given."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, None, True, state_d=state_d)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        Ed = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        Gd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_G else None
        self.call("sdp_sparsemax_adjoint_backward_f32", SPARSEMAX_ADJOINT_KERNELS[155], dev, state, state_d, Et, Ed, Gd, B, N, M, lens,
                  self._sparsemax_variant(variant))
        return Ed, Gd

    # ---- the affine-gap soft local operator (include/sdp.h: sdp_affine_local_*) ----------------
    def affine_local_forward(self, theta, gap_open, gap_extend, lens=None, state_out=None):
        """-> (Vt (B,), state): the affine-gap soft local sweep and its 48-byte records (opaque float32 tensor of
        sdp_affine_local_state_bytes).  state_out: a buffer of that size to write into instead of a fresh one."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nfloats = max(self.lib.sdp_affine_local_state_bytes(B, N, M), 4) // 4
        check_args(theta, torch.float32, (nfloats,), True, ValueError, state_out=state_out)
        state = torch.empty(nfloats, dtype=torch.float32, device=theta.device) if state_out is None else state_out
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_local_forward_f32", AFFINE_LOCAL_KERNELS[160], dev, theta, gap_open, gap_extend, state, Vt, B, N, M, lens, 0)
        return Vt, state

    def affine_local_forward_value(self, theta, gap_open, gap_extend, lens=None):
        """-> Vt (B,) alone: the same sweep with the records compiled out (the same bits); nothing else is allocated."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_local_forward_value_f32", AFFINE_LOCAL_KERNELS[161], dev, theta, gap_open, gap_extend, Vt, B, N, M, lens, 0)
        return Vt

    def affine_local_backward(self, state, Vt, Et, shape, lens=None, want_GO=True, want_GX=True):
        """The mirror sweep over the records of affine_local_forward -> (E (B,N,M), GO (B,N,M) or None, GX (B,N,M) or None):
        Et . dVt/dtheta, Et . dVt/dgap_open and Et . dVt/dgap_extend, +0 outside each pair's block.  Vt: what
        affine_local_forward returned with `state`."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        E = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        GO = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GO else None
        GX = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GX else None
        self.call("sdp_affine_local_backward_f32", AFFINE_LOCAL_KERNELS[162], dev, state, Vt, Et, E, GO, GX, B, N, M, lens, 0)
        return E, GO, GX

    def affine_local_adjoint_forward(self, state, Vt, ZE, ZGO, ZGX, shape, lens=None, state_d_out=None):
        """The adjoint forward sweep over the records of affine_local_forward -> (Vtd (B,), state_d): ZE, ZGO, ZGX (B,N,M) the
        cotangents of E, GO and GX, each may be None (zeros) but not all three; state_d the dot records (opaque float32 tensor of
        sdp_affine_local_adjoint_state_bytes; state_d_out: a buffer of that size to write into instead of a fresh one)."""
        dev = self.device_of(state)
        B, N, M = shape
        if ZE is None and ZGO is None and ZGX is None:
            raise ValueError("affine_local_adjoint_forward: ZE, ZGO and ZGX are all None")
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, torch.float32, (B, N, M), ZE=ZE, ZGO=ZGO, ZGX=ZGX)
        ZE, ZGO, ZGX = (None if z is None else z.detach().contiguous() for z in (ZE, ZGO, ZGX))
        lens = self._lens(lens, B, state.device)
        nfloats = max(self.lib.sdp_affine_local_adjoint_state_bytes(B, N, M), 4) // 4
        check_args(state, torch.float32, (nfloats,), True, ValueError, state_d_out=state_d_out)
        state_d = torch.empty(nfloats, dtype=torch.float32, device=state.device) if state_d_out is None else state_d_out
        Vtd = torch.empty(B, dtype=torch.float32, device=state.device)
        self.call("sdp_affine_local_adjoint_forward_f32", AFFINE_LOCAL_ADJOINT_KERNELS[167], dev, state, Vt, ZE, ZGO, ZGX, state_d, Vtd,
                  B, N, M, lens, 0)
        return Vtd, state_d

    def affine_local_adjoint_backward(self, state, state_d, Vt, Vtd, Et, shape, lens=None, want_GO=True, want_GX=True):
        """The adjoint mirror sweep -> (Ed (B,N,M), GOd (B,N,M) or None, GXd (B,N,M) or None): the gradients of <ZE,E> + <ZGO,GO> +
        <ZGX,GX> with respect to theta, gap_open and gap_extend, +0 outside each pair's block.  state, Vt: of affine_local_forward;
        state_d, Vtd: of affine_local_adjoint_forward; Et: what affine_local_backward was given."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt, Vtd=Vtd)
        check_args(state, torch.float32, None, True, state_d=state_d)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        Ed = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        GOd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GO else None
        GXd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GX else None
        self.call("sdp_affine_local_adjoint_backward_f32", AFFINE_LOCAL_ADJOINT_KERNELS[168], dev, state, state_d, Vt, Vtd, Et, Ed, GOd,
                  GXd, B, N, M, lens, 0)
        return Ed, GOd, GXd

    # ---- alignments sampled from its posterior (include/sdp.h: sdp_affine_local_end_tables_f32, sdp_affine_local_sample_paths_f32) ----
    def affine_local_end_tables(self, state, Vt, shape, lens=None, cdf_out=None, rows_out=None):
        """The end-cell tables over the records of affine_local_forward -> (cdf (B,N,M), rows (B,N+1)) fp32: the running sums of
        (w_x + w_y) + w_m, w_s = exp(V_s - Vt), along every row, and of the rows' totals from exp(-Vt) on.  Only entries inside a
        pair's block are written; fresh tensors are zero outside.  cdf_out / rows_out: buffers to write into instead of fresh ones."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, torch.float32, (B, N, M), True, ValueError, cdf_out=cdf_out)
        check_args(state, torch.float32, (B, N + 1), True, ValueError, rows_out=rows_out)
        lens = self._lens(lens, B, state.device)
        new = torch.empty if lens is None else torch.zeros      # (without lengths every entry is written)
        cdf = new((B, N, M), dtype=torch.float32, device=state.device) if cdf_out is None else cdf_out
        rows = new((B, N + 1), dtype=torch.float32, device=state.device) if rows_out is None else rows_out
        self.call("sdp_affine_local_end_tables_f32", AFFINE_LOCAL_SAMPLE_KERNELS[164], dev, state, Vt, cdf, rows, B, N, M, lens, 0)
        return cdf, rows

    def affine_local_sample_paths(self, state, Vt, cdf, rows, shape, K, lens=None, seed=0, sample0=0, want_states=True,
                                  want_visits=False, want_opens=False, want_extends=False, want_ends=False):
        """K local alignments per pair drawn from the posterior, on the `state` and `Vt` of affine_local_forward and the tables of
        affine_local_end_tables -> (states (B,K,cap,3) int32 or None, counts (B,K) int32 or None, visits, opens, extends (B,N,M)
        int32 or None, ends (B,K,3) int32 or None).  Sample (b, k) is sample number sample0 + k of pair b under `seed` whatever K
        is; its list -- the path alone, start first, rows (i, j, plane) -- is RIGHT-aligned in states[b, k]: rows
        cap-1-counts[b,k] .. cap-2, and row cap-1 holds (number of path cells, i, j of the first one), (0, -1, -1) for an empty
        sample; rows in front of the list are unspecified.  ends: the end cell and its plane, (-1, -1, -1) for an empty sample.
        visits: how many of the K paths pass through each cell; opens / extends: how many of them open / extend a gap into it."""
        dev = self.device_of(state)
        B, N, M = shape
        if not (want_states or want_visits or want_opens or want_extends or want_ends):
            raise ValueError("affine_local_sample_paths: nothing asked for (want_states, want_visits, want_opens, want_extends, want_ends)")
        check_args(state, torch.float32, (B,), True, Vt=Vt)
        check_args(state, torch.float32, (B, N, M), True, ValueError, cdf=cdf)
        check_args(state, torch.float32, (B, N + 1), True, ValueError, rows=rows)
        lens = self._lens(lens, B, state.device)
        states = counts = ends = None
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            states = torch.empty((B, int(K), cap, 3), dtype=torch.int32, device=state.device)
            counts = torch.empty((B, int(K)), dtype=torch.int32, device=state.device)
        visits, opens, extends = (torch.zeros((B, N, M), dtype=torch.int32, device=state.device) if want else None
                                  for want in (want_visits, want_opens, want_extends))
        if want_ends:
            ends = torch.empty((B, int(K), 3), dtype=torch.int32, device=state.device)
        self.call("sdp_affine_local_sample_paths_f32", AFFINE_LOCAL_SAMPLE_KERNELS[165], dev, state, Vt, cdf, rows, states, counts, visits,
                  opens, extends, ends, B, N, M, int(K), int(sample0), int(seed) & 0xffffffffffffffff, lens, 0)
        return states, counts, visits, opens, extends, ends

    # ---- the affine-gap soft global operator (include/sdp.h: sdp_affine_global_*) ---------------
    def affine_global_forward(self, theta, gap_open, gap_extend, lens=None, state_out=None):
        """-> (Vt (B,), state): the affine-gap soft global sweep and its 48-byte records (opaque float32 tensor of
        sdp_affine_global_state_bytes; the end weights travel in it).  state_out: a buffer of that size to write into instead of a
        fresh one."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nfloats = max(self.lib.sdp_affine_global_state_bytes(B, N, M), 4) // 4
        check_args(theta, torch.float32, (nfloats,), True, ValueError, state_out=state_out)
        state = torch.empty(nfloats, dtype=torch.float32, device=theta.device) if state_out is None else state_out
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_global_forward_f32", AFFINE_GLOBAL_KERNELS[180], dev, theta, gap_open, gap_extend, state, Vt, B, N, M, lens, 0)
        return Vt, state

    def affine_global_forward_value(self, theta, gap_open, gap_extend, lens=None):
        """-> Vt (B,) alone: the same sweep with the records compiled out (the same bits); nothing else is allocated."""
        dev = self.device_of(theta)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_global_forward_value_f32", AFFINE_GLOBAL_KERNELS[181], dev, theta, gap_open, gap_extend, Vt, B, N, M, lens, 0)
        return Vt

    def affine_global_backward(self, state, Et, shape, lens=None, want_GO=True, want_GX=True):
        """The mirror sweep over the records of affine_global_forward -> (E (B,N,M), GO (B,N,M) or None, GX (B,N,M) or None):
        Et . dVt/dtheta, Et . dVt/dgap_open and Et . dVt/dgap_extend, +0 outside each pair's block.  (No Vt: the end weights are in
        `state`.)"""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, None, True, state=state)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        E = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        GO = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GO else None
        GX = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GX else None
        self.call("sdp_affine_global_backward_f32", AFFINE_GLOBAL_KERNELS[182], dev, state, Et, E, GO, GX, B, N, M, lens, 0)
        return E, GO, GX

    # ---- its free-end-gap member (include/sdp.h: sdp_affine_semiglobal_*) ---------------
    @staticmethod
    def _free_ends(free_ends):
        free_ends = int(free_ends)
        if free_ends & ~3:
            raise ValueError(f"free_ends must be 0 .. 3 (bit 0: x, bit 1: y), got {free_ends}")
        return free_ends

    def affine_semiglobal_forward(self, theta, gap_open, gap_extend, free_ends, lens=None, state_out=None):
        """-> (Vt (B,), state): affine_global_forward with free end gaps -- free_ends bit 0: x (rows may hang over), bit 1: y
        (columns); 0: the global operator's bits.  state: opaque float32 tensor of sdp_affine_semiglobal_state_bytes (the global
        records and a tail of end-cell exponents; the end weights travel in it)."""
        dev = self.device_of(theta)
        free_ends = self._free_ends(free_ends)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nfloats = max(self.lib.sdp_affine_semiglobal_state_bytes(B, N, M), 4) // 4
        check_args(theta, torch.float32, (nfloats,), True, ValueError, state_out=state_out)
        state = torch.empty(nfloats, dtype=torch.float32, device=theta.device) if state_out is None else state_out
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_semiglobal_forward_f32", AFFINE_SEMIGLOBAL_KERNELS[200], dev, theta, gap_open, gap_extend, state, Vt, B, N, M,
                  lens, free_ends, 0)
        return Vt, state

    def affine_semiglobal_forward_value(self, theta, gap_open, gap_extend, free_ends, lens=None):
        """-> Vt (B,) alone: the same sweep with the records and the tail compiled out (the same bits); nothing else is allocated."""
        dev = self.device_of(theta)
        free_ends = self._free_ends(free_ends)
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        theta, gap_open, gap_extend = theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        self.call("sdp_affine_semiglobal_forward_value_f32", AFFINE_SEMIGLOBAL_KERNELS[201], dev, theta, gap_open, gap_extend, Vt, B, N, M,
                  lens, free_ends, 0)
        return Vt

    def affine_semiglobal_backward(self, state, Et, shape, free_ends, lens=None, want_GO=True, want_GX=True):
        """The mirror sweep over the records of affine_semiglobal_forward (the same free_ends) -> (E (B,N,M), GO (B,N,M) or None,
        GX (B,N,M) or None), +0 outside each pair's block.  (No Vt: the end weights are in `state`.)"""
        dev = self.device_of(state)
        free_ends = self._free_ends(free_ends)
        B, N, M = shape
        check_args(state, torch.float32, None, True, state=state)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        E = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        GO = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GO else None
        GX = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GX else None
        self.call("sdp_affine_semiglobal_backward_f32", AFFINE_SEMIGLOBAL_KERNELS[202], dev, state, Et, E, GO, GX, B, N, M, lens, free_ends, 0)
        return E, GO, GX

    # ---- alignments sampled from its posterior (include/sdp.h: sdp_affine_semiglobal_end_table_f32, .._sample_paths_f32) ----
    def affine_semiglobal_end_table(self, state, shape, free_ends, lens=None):
        """-> ecdf (B, N + M) float32: the running sums of the end cells' weights of every pair, on the `state` of
        affine_semiglobal_forward under the same free_ends and lens -- candidate e < n_b is cell (e, m_b - 1), e >= n_b cell
        (n_b - 1, e - n_b); a cell that is no end cell under free_ends weighs exactly 0.  Entries from n_b + m_b - 1 on are not
        written.  One table serves any number of affine_semiglobal_sample_paths launches (a K split by sample0)."""
        dev = self.device_of(state)
        free_ends = self._free_ends(free_ends)
        B, N, M = shape
        check_args(state, torch.float32, None, True, state=state)
        lens = self._lens(lens, B, state.device)
        ecdf = torch.empty((B, N + M), dtype=torch.float32, device=state.device)
        self.call("sdp_affine_semiglobal_end_table_f32", AFFINE_SEMIGLOBAL_SAMPLE_KERNELS[211], dev, state, ecdf, B, N, M, lens,
                  free_ends, 0)
        return ecdf

    def affine_semiglobal_sample_paths(self, state, ecdf, shape, free_ends, K, lens=None, seed=0, sample0=0, want_states=True,
                                       want_visits=False, want_opens=False, want_extends=False, want_ends=False):
        """K semi-global alignments per pair drawn from the posterior, on the `state` of affine_semiglobal_forward and the `ecdf` of
        affine_semiglobal_end_table (the same free_ends and lens) -> (states (B,K,cap,3) int32 or None, counts (B,K) int32 or None,
        visits, opens, extends (B,N,M) int32 or None, ends (B,K,3) int32 or None), in the formats of affine_global_sample_paths:
        the list of sample (b, k) -- sample number sample0 + k of pair b under `seed` whatever K is -- runs from a start cell to
        the drawn end cell, rows (i, j, plane), RIGHT-aligned in states[b, k]; row cap-1 holds (number of path cells, i, j of the
        first one), (0, -1, -1) for an empty sample -- an empty pair, or a pair without a path.  ends: (i, j, plane) of the end
        cell, (-1, -1, -1) for an empty sample."""
        dev = self.device_of(state)
        free_ends = self._free_ends(free_ends)
        B, N, M = shape
        if not (want_states or want_visits or want_opens or want_extends or want_ends):
            raise ValueError("affine_semiglobal_sample_paths: nothing asked for (want_states, want_visits, want_opens, want_extends, "
                             "want_ends)")
        check_args(state, torch.float32, None, True, state=state)
        check_args(state, torch.float32, (B, N + M), True, ecdf=ecdf)
        lens = self._lens(lens, B, state.device)
        states = counts = ends = None
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            states = torch.empty((B, int(K), cap, 3), dtype=torch.int32, device=state.device)
            counts = torch.empty((B, int(K)), dtype=torch.int32, device=state.device)
        visits, opens, extends = (torch.zeros((B, N, M), dtype=torch.int32, device=state.device) if want else None
                                  for want in (want_visits, want_opens, want_extends))
        if want_ends:
            ends = torch.empty((B, int(K), 3), dtype=torch.int32, device=state.device)
        self.call("sdp_affine_semiglobal_sample_paths_f32", AFFINE_SEMIGLOBAL_SAMPLE_KERNELS[212], dev, state, ecdf, states, counts,
                  visits, opens, extends, ends, B, N, M, int(K), int(sample0), int(seed) & 0xffffffffffffffff, lens, free_ends, 0)
        return states, counts, visits, opens, extends, ends

    def affine_global_adjoint_forward(self, state, ZE, ZGO, ZGX, shape, lens=None, state_d_out=None):
        """The adjoint forward sweep over the records of affine_global_forward -> (Vtd (B,), state_d): ZE, ZGO, ZGX (B,N,M) the
        cotangents of E, GO and GX, each may be None (zeros) but not all three; state_d the dot records (opaque float32 tensor of
        sdp_affine_global_adjoint_state_bytes; state_d_out: a buffer of that size to write into instead of a fresh one).  (No Vt:
        the end weights are in `state`.)"""
        dev = self.device_of(state)
        B, N, M = shape
        if ZE is None and ZGO is None and ZGX is None:
            raise ValueError("affine_global_adjoint_forward: ZE, ZGO and ZGX are all None")
        check_args(state, torch.float32, None, True, state=state)
        check_args(state, torch.float32, (B, N, M), ZE=ZE, ZGO=ZGO, ZGX=ZGX)
        ZE, ZGO, ZGX = (None if z is None else z.detach().contiguous() for z in (ZE, ZGO, ZGX))
        lens = self._lens(lens, B, state.device)
        nfloats = max(self.lib.sdp_affine_global_adjoint_state_bytes(B, N, M), 4) // 4
        check_args(state, torch.float32, (nfloats,), True, ValueError, state_d_out=state_d_out)
        state_d = torch.empty(nfloats, dtype=torch.float32, device=state.device) if state_d_out is None else state_d_out
        Vtd = torch.empty(B, dtype=torch.float32, device=state.device)
        self.call("sdp_affine_global_adjoint_forward_f32", AFFINE_GLOBAL_ADJOINT_KERNELS[193], dev, state, ZE, ZGO, ZGX, state_d, Vtd,
                  B, N, M, lens, 0)
        return Vtd, state_d

    def affine_global_adjoint_backward(self, state, state_d, Vtd, Et, shape, lens=None, want_GO=True, want_GX=True):
        """The adjoint mirror sweep -> (Ed (B,N,M), GOd (B,N,M) or None, GXd (B,N,M) or None): the gradients of <ZE,E> + <ZGO,GO> +
        <ZGX,GX> with respect to theta, gap_open and gap_extend, +0 outside each pair's block.  state: of affine_global_forward;
        state_d, Vtd: of affine_global_adjoint_forward; Et: what affine_global_backward was given."""
        dev = self.device_of(state)
        B, N, M = shape
        check_args(state, torch.float32, (B,), True, Vtd=Vtd)
        check_args(state, torch.float32, None, True, state_d=state_d)
        check_args(state, Et=Et)
        Et = Et.detach().to(torch.float32).expand(B).contiguous()
        lens = self._lens(lens, B, state.device)
        Ed = torch.empty((B, N, M), dtype=torch.float32, device=state.device)
        GOd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GO else None
        GXd = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if want_GX else None
        self.call("sdp_affine_global_adjoint_backward_f32", AFFINE_GLOBAL_ADJOINT_KERNELS[194], dev, state, state_d, Vtd, Et, Ed, GOd, GXd,
                  B, N, M, lens, 0)
        return Ed, GOd, GXd

    # ---- alignments sampled from its posterior (include/sdp.h: sdp_affine_global_sample_paths_f32) ----
    def affine_global_sample_paths(self, state, shape, K, lens=None, seed=0, sample0=0, want_states=True, want_visits=False,
                                   want_opens=False, want_extends=False, want_ends=False):
        """K global alignments per pair drawn from the posterior, on the `state` of affine_global_forward (the end weights are in
        it: no Vt, no tables) -> (states (B,K,cap,3) int32 or None, counts (B,K) int32 or None, visits, opens, extends (B,N,M)
        int32 or None, ends (B,K,3) int32 or None), in the formats of affine_local_sample_paths: the list of sample (b, k) -- sample
        number sample0 + k of pair b under `seed` whatever K is -- runs from cell (0, 0) to cell (n_b - 1, m_b - 1), rows (i, j,
        plane), RIGHT-aligned in states[b, k]: rows cap-1-counts[b,k] .. cap-2, and row cap-1 holds (number of path cells, i, j of
        the first one), (0, -1, -1) for an empty sample -- an empty pair, or a pair without a path; rows in front of the list are
        unspecified.  ends: (n_b - 1, m_b - 1, the end plane), (-1, -1, -1) for an empty sample.  visits: how many of the K paths
        pass through each cell; opens / extends: how many of them open / extend a gap into it."""
        dev = self.device_of(state)
        B, N, M = shape
        if not (want_states or want_visits or want_opens or want_extends or want_ends):
            raise ValueError("affine_global_sample_paths: nothing asked for (want_states, want_visits, want_opens, want_extends, want_ends)")
        check_args(state, torch.float32, None, True, state=state)
        lens = self._lens(lens, B, state.device)
        states = counts = ends = None
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            states = torch.empty((B, int(K), cap, 3), dtype=torch.int32, device=state.device)
            counts = torch.empty((B, int(K)), dtype=torch.int32, device=state.device)
        visits, opens, extends = (torch.zeros((B, N, M), dtype=torch.int32, device=state.device) if want else None
                                  for want in (want_visits, want_opens, want_extends))
        if want_ends:
            ends = torch.empty((B, int(K), 3), dtype=torch.int32, device=state.device)
        self.call("sdp_affine_global_sample_paths_f32", AFFINE_GLOBAL_SAMPLE_KERNELS[190], dev, state, states, counts, visits, opens,
                  extends, ends, B, N, M, int(K), int(sample0), int(seed) & 0xffffffffffffffff, lens, 0)
        return states, counts, visits, opens, extends, ends

    # ---- the hard affine-gap local operator (include/sdp.h: sdp_hard_affine_local_*) ------------
    def _hard_affine_variant(self, ymx, waves=True):
        """`variant` of the sdp_hard_affine_local_* entries; waves=False for the walk, which runs one wave per pair."""
        w = self.force_waves.get("hard_affine", 0) if waves else 0
        return (_lib.SDP_HARD_TIES_YMX if ymx else 0) | (_lib.SDP_WAVES(w) if w else 0)

    def _hard_affine_inputs(self, theta, gap_open, gap_extend):
        check_args(theta, torch.float32, theta=theta, gap_open=gap_open, gap_extend=gap_extend)
        check_args(theta, None, tuple(theta.shape), gap_open=gap_open, gap_extend=gap_extend)
        return theta.contiguous(), gap_open.contiguous(), gap_extend.contiguous()

    def hard_affine_local_forward(self, theta, gap_open, gap_extend, lens=None, ymx=False):
        """-> (Vt (B,), state, ends (B, 3) int32): the Gotoh max-plus sweep -- Vt the best plane value, ends its 0-based (i, j) and
        plane, (-1, -1, -1) where nothing is positive -- and its 2-bit pointers, three planes (opaque int32 tensor of
        sdp_hard_affine_local_state_bytes).  ymx: the tensors are a TRANSPOSED problem; ends come back in the coordinates and
        plane names handed over."""
        return self._hard_affine_forward("local", HARD_AFFINE_LOCAL_KERNELS, 170, theta, gap_open, gap_extend, lens, ymx)

    def _hard_affine_forward(self, member, kernels, first, theta, gap_open, gap_extend, lens, ymx, extra=()):
        """the pointer sweep of sdp_hard_affine_<member>_*; kernels[first], kernels[first + 1]: its two tie orders; extra: the
        entry's arguments between lens and variant (the semi-global member's free_ends)"""
        dev = self.device_of(theta)
        theta, gap_open, gap_extend = self._hard_affine_inputs(theta, gap_open, gap_extend)
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        nbytes = getattr(self.lib, f"sdp_hard_affine_{member}_state_bytes")(B, N, M)
        state = torch.empty(max(nbytes, 4) // 4, dtype=torch.int32, device=theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        ends = torch.empty((B, 3), dtype=torch.int32, device=theta.device)
        self.call(f"sdp_hard_affine_{member}_forward_f32", kernels[first + (1 if ymx else 0)], dev, theta, gap_open, gap_extend,
                  state, Vt, ends, B, N, M, lens, *extra, self._hard_affine_variant(ymx))
        return Vt, state, ends

    def hard_affine_local_forward_value(self, theta, gap_open, gap_extend, lens=None, ymx=False, want_ends=True):
        """-> (Vt (B,), ends (B, 3) int32 or None): the same sweep with the pointers compiled out (the same bits)."""
        return self._hard_affine_forward_value("local", HARD_AFFINE_LOCAL_KERNELS, 172, theta, gap_open, gap_extend, lens, ymx, want_ends)

    def _hard_affine_forward_value(self, member, kernels, first, theta, gap_open, gap_extend, lens, ymx, want_ends, extra=()):
        dev = self.device_of(theta)
        theta, gap_open, gap_extend = self._hard_affine_inputs(theta, gap_open, gap_extend)
        B, N, M = theta.shape
        lens = self._lens(lens, B, theta.device)
        Vt = torch.empty(B, dtype=torch.float32, device=theta.device)
        ends = torch.empty((B, 3), dtype=torch.int32, device=theta.device) if want_ends else None
        self.call(f"sdp_hard_affine_{member}_forward_value_f32", kernels[first + (1 if ymx else 0)], dev, theta, gap_open,
                  gap_extend, Vt, ends, B, N, M, lens, *extra, self._hard_affine_variant(ymx))
        return Vt, ends

    def hard_affine_local_walk(self, state, ends, shape, lens=None, Et=None, ymx=False, want_E=True, want_GO=False, want_GX=False,
                               want_states=True, E_out=None, GO_out=None, GX_out=None, states_out=None, entry="sdp_hard_affine_local_walk_f32"):
        """The walk along the pointers of hard_affine_local_forward, from `ends` -> (E, GO, GX (B,N,M) or None each, states
        (B,cap,3) int32 or None, counts (B,) or None).  E: Et[b] on pair b's path, GO / GX: Et[b] on its gap cells entered from
        another plane / the same plane, +0 on every other cell of the plane; states / counts: the path alone (no padding), start
        first; row cap - 1 of states: (number of path cells, i and j of its first cell).  *_out: buffers to write into.
        entry: the C entry to go through (hard_affine_global_walk names its own; the kernel is the same)."""
        dev = self.device_of(state)
        B, N, M = shape
        lens = self._lens(lens, B, state.device)
        check_args(state, torch.int32, (B, 3), True, ValueError, ends=ends)
        planes = [None, None, None]
        states = counts = None
        wants = (want_E, want_GO, want_GX)
        if any(wants):
            if Et is None:
                raise ValueError("hard_affine_local_walk: E, GO and GX need Et")
            check_args(state, Et=Et)
            Et = Et.detach().to(torch.float32).expand(B).contiguous()
            check_args(state, torch.float32, (B, N, M), True, ValueError, E_out=E_out, GO_out=GO_out, GX_out=GX_out)
            for k, (want, buf) in enumerate(zip(wants, (E_out, GO_out, GX_out))):
                if want:
                    planes[k] = torch.empty((B, N, M), dtype=torch.float32, device=state.device) if buf is None else buf
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            check_args(state, torch.int32, (B, cap, 3), True, ValueError, states_out=states_out)
            states = torch.empty((B, cap, 3), dtype=torch.int32, device=state.device) if states_out is None else states_out
            counts = torch.empty(B, dtype=torch.int32, device=state.device)
        self.call(entry, HARD_AFFINE_LOCAL_KERNELS[174], dev, state, ends, Et if any(wants) else None, *planes,
                  states, counts, B, N, M, lens, self._hard_affine_variant(ymx, waves=False))
        return planes[0], planes[1], planes[2], states, counts

    # ---- the hard affine-gap global operator (include/sdp.h: sdp_hard_affine_global_*): the local member's launches ----
    def hard_affine_global_forward(self, theta, gap_open, gap_extend, lens=None, ymx=False):
        """-> (Vt (B,), state, ends (B, 3) int32): the Gotoh max-plus sweep from cell (0, 0) to cell (n - 1, m - 1) -- Vt the first
        maximum of the last cell's planes, -inf for a pair without a path, +0 for an empty pair; ends (n - 1, m - 1, plane),
        (-1, -1, -1) where there is no path -- and its pointers in the local member's format.  ymx: as hard_affine_local_forward."""
        return self._hard_affine_forward("global", HARD_AFFINE_GLOBAL_KERNELS, 185, theta, gap_open, gap_extend, lens, ymx)

    def hard_affine_global_forward_value(self, theta, gap_open, gap_extend, lens=None, ymx=False, want_ends=True):
        """-> (Vt (B,), ends (B, 3) int32 or None): the same sweep with the pointers compiled out (the same bits)."""
        return self._hard_affine_forward_value("global", HARD_AFFINE_GLOBAL_KERNELS, 187, theta, gap_open, gap_extend, lens, ymx, want_ends)

    def hard_affine_global_walk(self, state, ends, shape, lens=None, **kw):
        """hard_affine_local_walk on the pointers of hard_affine_global_forward (the state format, ends and the stop at START are the
        same), through sdp_hard_affine_global_walk_f32."""
        return self.hard_affine_local_walk(state, ends, shape, lens, entry="sdp_hard_affine_global_walk_f32", **kw)

    # ---- the hard affine-gap semi-global operator (include/sdp.h: sdp_hard_affine_semiglobal_*): free end gaps ----
    def _hard_affine_semiglobal(self, free_ends, first):
        """-> (free_ends checked, the kernel table and the id of the first of the two tie orders a launch under it takes:
        free_ends = 0 is the global member and launches its kernels)"""
        free_ends = self._free_ends(free_ends)
        if free_ends == 0:
            return free_ends, HARD_AFFINE_GLOBAL_KERNELS, first - 20
        return free_ends, HARD_AFFINE_SEMIGLOBAL_KERNELS, first

    def hard_affine_semiglobal_forward(self, theta, gap_open, gap_extend, free_ends, lens=None, ymx=False):
        """-> (Vt (B,), state, ends (B, 3) int32): hard_affine_global_forward with free end gaps -- free_ends bit 0: x (rows may hang
        over: a path starts in column 0 and ends in column m - 1), bit 1: y (columns: row 0 and row n - 1); 0: the global member's
        bits.  Vt the first maximum over the end cells and their planes, -inf for a pair without a path, +0 for an empty pair; ends
        its 0-based cell and plane, (-1, -1, -1) where there is no path; the pointers in the local member's format.  ymx: the
        tensors are a TRANSPOSED problem and free_ends its swapped bits; ends come back in the coordinates and plane names handed
        over."""
        free_ends, kernels, first = self._hard_affine_semiglobal(free_ends, 205)
        return self._hard_affine_forward("semiglobal", kernels, first, theta, gap_open, gap_extend, lens, ymx, extra=(free_ends,))

    def hard_affine_semiglobal_forward_value(self, theta, gap_open, gap_extend, free_ends, lens=None, ymx=False, want_ends=True):
        """-> (Vt (B,), ends (B, 3) int32 or None): the same sweep with the pointers compiled out (the same bits)."""
        free_ends, kernels, first = self._hard_affine_semiglobal(free_ends, 207)
        return self._hard_affine_forward_value("semiglobal", kernels, first, theta, gap_open, gap_extend, lens, ymx, want_ends,
                                               extra=(free_ends,))

    def hard_affine_semiglobal_walk(self, state, ends, shape, lens=None, **kw):
        """hard_affine_local_walk on the pointers of hard_affine_semiglobal_forward (the state format, ends and the stop at START
        are the same: the walk stops in the start cell wherever that is), through sdp_hard_affine_semiglobal_walk_f32."""
        return self.hard_affine_local_walk(state, ends, shape, lens, entry="sdp_hard_affine_semiglobal_walk_f32", **kw)

    # ---- alignments sampled from the posterior (include/sdp.h: sdp_sample_paths_*) -------------------
    def sample_paths(self, state, shape, variant, K, lens=None, seed=0, sample0=0, exact_state=False, transposed=False,
                     want_states=True, want_visits=False):
        """K stochastic tracebacks per pair on the `state` of forward() -> (states (B,K,cap,3) int32 or None, counts (B,K) int32 or
        None, visits (B,N,M) int32 or None).  exact_state, lens: what forward() was given (a float64 state is known by its dtype).
        Sample (b, k) is sample number sample0 + k of pair b under `seed` whatever K is; its list is RIGHT-aligned in
        states[b, k] -- rows cap-1-counts[b,k] .. cap-2, start first -- and row cap-1 holds (number of path cells, i, j of the
        first one).  visits: how many of the K paths pass through each cell.  transposed: the state is that of a transposed
        problem (_Decoder._oriented); (i, j) stay in the state's coordinates."""
        dev = self.device_of(state)
        B, N, M = shape
        if not want_states and not want_visits:
            raise ValueError("sample_paths: nothing asked for (want_states, want_visits)")
        lens = self._lens(lens, B, state.device)
        states = counts = visits = None
        if want_states:
            cap = self.lib.sdp_traceback_capacity(N, M)
            states = torch.empty((B, int(K), cap, 3), dtype=torch.int32, device=state.device)
            counts = torch.empty((B, int(K)), dtype=torch.int32, device=state.device)
        if want_visits:
            visits = torch.zeros((B, N, M), dtype=torch.int32, device=state.device)
        flags = _lib.SDP_SAMPLE_TRANSPOSED if transposed else 0
        seed = int(seed) & 0xffffffffffffffff
        if _sweep_dtype(state) == torch.float64:
            check_args(state, torch.float64, (B, N, M, 3), True, state=state)
            self.call("sdp_sample_paths_f64", "sdp_sample_rows_f64_kernel", dev, state, states, counts, visits, B, N, M, int(K),
                      int(sample0), seed, lens, variant | flags)
        else:
            flags |= self._state_flags(exact_state)
            self.call("sdp_sample_paths_f32", "sdp_sample_rows_kernel" if exact_state == REF else "sdp_sample_kernel", dev,
                      state, states, counts, visits, B, N, M, int(K), int(sample0), seed, lens, variant | flags)
        return states, counts, visits

    def alignment_targets(self, codes, code_lens, lens, shape, dm, P, G, flags, status):
        """Enqueue sdp_alignment_targets on the current stream (include/sdp.h): codes (B, L) uint8, code_lens (B,) int32,
        lens (B, 2) int32 or None; dm / P fp32, G bool or fp32 (flags), each (B, N, M) or None; status (B,) int32."""
        dev = self.device_of(codes)
        B, N, M = shape
        check_args(codes, None, (B, N, M), True, dm=dm, P=P, G=G)
        self.call("sdp_alignment_targets", "sdp_targets_kernel", dev, codes, code_lens, codes.shape[1], lens, B, N, M, dm, P, G, flags, status)
        return status

    def alignment_stats(self, true_codes, true_lens, pred, pred_lens, offsets, widths, flags, counts, stats, hits, identity,
                        status):
        """Enqueue sdp_alignment_stats on the current stream (include/sdp.h): true_codes (B, Lt) uint8, true_lens (B,) int32;
        pred (B, Lp) uint8 codes, or with SDP_SCORE_PRED_WALK the walk (B, cap, 3) int32, pred_lens (B,) int32 (its counts);
        offsets (B, 2) int32 or None; widths (W,) int32 or None; counts (B, 5) int32; stats (B, 7) float64, hits (B, W)
        int32, identity (B, W) float64, each or None; status (B,) int32.  Every tensor contiguous on one device."""
        dev = self.device_of(true_codes)
        B, Lt = true_codes.shape
        Lp = pred.shape[1]
        W = 0 if widths is None else widths.numel()
        walk = flags & _lib.SDP_SCORE_PRED_WALK
        for dtype, shape, tensors in ((torch.uint8, (B, Lt), {"true_codes": true_codes}),
                                     (torch.int32 if walk else torch.uint8, (B, Lp, 3) if walk else (B, Lp), {"pred": pred}),
                                     (torch.int32, (B,), {"true_lens": true_lens, "pred_lens": pred_lens, "status": status}),
                                     (torch.int32, (B, 2), {"offsets": offsets}), (torch.int32, (W,), {"widths": widths}),
                                     (torch.int32, (B, 5), {"counts": counts}), (torch.float64, (B, 7), {"stats": stats}),
                                     (torch.int32, (B, W), {"hits": hits}), (torch.float64, (B, W), {"identity": identity})):
            check_args(true_codes, dtype, shape, True, ValueError, **tensors)
        self.call("sdp_alignment_stats", "sdp_score_kernel", dev, true_codes, true_lens, Lt, pred, pred_lens, Lp, offsets, widths, W, B,
                  flags, counts, stats, hits, identity, status)
        return status

    def targets_selftest(self, device=0):
        _lib.check(self.lib.sdp_targets_selftest(device), "sdp_targets_selftest")

    def init(self, device=None):
        """Create the library's per-device state now (include/sdp.h: sdp_init) -- needed only before stream capture."""
        dev = torch.cuda.current_device() if device is None else device
        _lib.check(self.lib.sdp_init(dev), "sdp_init")

    def selftest(self, device=0):
        _lib.check(self.lib.sdp_selftest(device), "sdp_selftest")


# kernel id (csrc/sdp_hard.h; what sdp_kernel_name answers for) -> symbol of the local-alignment kernels: the launch labels
HARD_LOCAL_KERNELS = {110: "sdp_hard_local_fwd_kernel", 111: "sdp_hard_local_fwd_t_kernel", 112: "sdp_hard_local_val_kernel",
                      113: "sdp_hard_local_val_t_kernel", 114: "sdp_hard_local_walk_kernel"}
# kernel id (csrc/sdp_soft_local.h) -> symbol of the soft local operator's kernels
SOFT_LOCAL_KERNELS = {130: "sdp_soft_local_fwd_kernel", 131: "sdp_soft_local_val_kernel", 132: "sdp_soft_local_bwd_kernel"}
# the same of its adjoint pair (csrc/sdp_soft_local_adj.hip)
SOFT_LOCAL_ADJOINT_KERNELS = {140: "sdp_soft_local_adj_fwd_kernel", 141: "sdp_soft_local_adj_bwd_kernel"}
# and of the kernels that sample from its posterior (csrc/sdp_soft_local_sample.h)
SOFT_LOCAL_SAMPLE_KERNELS = {134: "sdp_soft_local_tables_kernel", 135: "sdp_soft_local_sample_kernel"}
# kernel id (csrc/sdp_sparsemax.h) -> symbol of the sparsemax operator's kernels
SPARSEMAX_KERNELS = {150: "sdp_sparsemax_fwd_kernel", 151: "sdp_sparsemax_val_kernel", 152: "sdp_sparsemax_bwd_kernel"}
# the same of its adjoint pair (csrc/sdp_sparsemax_adj.hip)
SPARSEMAX_ADJOINT_KERNELS = {154: "sdp_sparsemax_adj_fwd_kernel", 155: "sdp_sparsemax_adj_bwd_kernel"}
# kernel id (csrc/sdp_affine_global.h) -> symbol of the affine-gap soft global operator's kernels
AFFINE_GLOBAL_KERNELS = {180: "sdp_affine_global_fwd_kernel", 181: "sdp_affine_global_val_kernel", 182: "sdp_affine_global_bwd_kernel"}
# of its free-end-gap member (the same header; csrc/sdp_affine_semiglobal.hip)
AFFINE_SEMIGLOBAL_KERNELS = {200: "sdp_affine_semiglobal_fwd_kernel", 201: "sdp_affine_semiglobal_val_kernel",
                             202: "sdp_affine_semiglobal_bwd_kernel"}
# of the kernels that sample from the semi-global posterior (csrc/sdp_affine_semiglobal_sample.h)
AFFINE_SEMIGLOBAL_SAMPLE_KERNELS = {211: "sdp_affine_semiglobal_end_table_kernel", 212: "sdp_affine_semiglobal_sample_kernel"}
# of its adjoint pair (the same header)
AFFINE_GLOBAL_ADJOINT_KERNELS ={193: "sdp_affine_global_adj_fwd_kernel", 194: "sdp_affine_global_adj_bwd_kernel"}
# and of the kernel that samples from its posterior (csrc/sdp_affine_global_sample.h)
AFFINE_GLOBAL_SAMPLE_KERNELS = {190: "sdp_affine_global_sample_kernel"}
# kernel id (csrc/sdp_affine_local.h) -> symbol of the affine-gap soft local operator's kernels
AFFINE_LOCAL_KERNELS = {160: "sdp_affine_local_fwd_kernel", 161: "sdp_affine_local_val_kernel", 162: "sdp_affine_local_bwd_kernel"}
# of its adjoint pair (the same header)
AFFINE_LOCAL_ADJOINT_KERNELS = {167: "sdp_affine_local_adj_fwd_kernel", 168: "sdp_affine_local_adj_bwd_kernel"}
# and of the kernels that sample from its posterior (csrc/sdp_affine_local_sample.h)
AFFINE_LOCAL_SAMPLE_KERNELS = {164: "sdp_affine_local_tables_kernel", 165: "sdp_affine_local_sample_kernel"}
# kernel id (csrc/sdp_hard_affine.h) -> symbol of the hard affine-gap local operator's kernels
HARD_AFFINE_LOCAL_KERNELS = {170: "sdp_hard_affine_local_fwd_kernel", 171: "sdp_hard_affine_local_fwd_t_kernel",
                             172: "sdp_hard_affine_local_val_kernel", 173: "sdp_hard_affine_local_val_t_kernel",
                             174: "sdp_hard_affine_local_walk_kernel"}
# the sweeps of its global member (the same header); the walk is kernel 174
HARD_AFFINE_GLOBAL_KERNELS = {185: "sdp_hard_affine_global_fwd_kernel", 186: "sdp_hard_affine_global_fwd_t_kernel",
                              187: "sdp_hard_affine_global_val_kernel", 188: "sdp_hard_affine_global_val_t_kernel"}
# and of its semi-global member, free end gaps (the same header); the walk is kernel 174
HARD_AFFINE_SEMIGLOBAL_KERNELS = {205: "sdp_hard_affine_semiglobal_fwd_kernel", 206: "sdp_hard_affine_semiglobal_fwd_t_kernel",
                                  207: "sdp_hard_affine_semiglobal_val_kernel", 208: "sdp_hard_affine_semiglobal_val_t_kernel"}

_SWEEPS = ("sdp_forward", "sdp_backward", "sdp_adjoint_forward", "sdp_adjoint_backward")
# dtype -> (suffix of the four sweeps' entries, their launch labels (float32: where the library's plan is not asked),
#           allocator of Q / Qd: (engine, B, N, M, device, derivative=, ref=))
_PRECISIONS = {
    torch.float32: ("_f32", ("sdp_fwd_kernel", "sdp_bwd_kernel", "sdp_adj_fwd_kernel", "sdp_adj_bwd_kernel"), HipEngine.new_state),
    torch.float64: ("_f64", ("sdp_f64_fwd_kernel", "sdp_f64_bwd_kernel", "sdp_f64_adj_fwd_kernel", "sdp_f64_adj_bwd_kernel"),
                    lambda eng, B, N, M, device, **_: torch.empty((B, N, M, 3), dtype=torch.float64, device=device)),
}

_ENGINE = None


def get_engine():
    """The process-wide engine.  Raises (ImportError) if the HIP library is not built."""
    global _ENGINE
    if _ENGINE is None:
        _ENGINE = HipEngine()
    return _ENGINE
