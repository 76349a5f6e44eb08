"""ctypes binding of libaigar_hip.so (include/aigar.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded
this module raises, so a GPU run can never silently take another path.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("AIGAR_SO") or os.path.join(HERE, "libaigar_hip.so")  # (AIGAR_SO: diagnostics builds)

_lib = None


def _preload_single_hip_runtime():
    """torch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP
    runtimes in one process break each other (and make torch streams invalid
    handles for us), so when torch is installed we bind to ITS runtime: preload
    it by path, before our library resolves libamdhip64.so.7.  torch imported
    later resolves to the same file."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)
        return cand
    return None


def rccl_path():
    """The librccl.so this process's torch uses (one HIP runtime for both), else None
    (the loader's librccl.so)."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is not None and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
        if os.path.exists(cand):
            return cand
    return None


def rccl_unique_id():
    """A fresh ncclUniqueId (128 bytes) for aigar_tile_comm_init (rank 0 makes it)."""
    L = load()
    buf = C.create_string_buffer(128)
    path = rccl_path()
    if L.aigar_rccl_unique_id(path.encode() if path else None, buf) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())
    return buf.raw


def load(build_if_missing=False):
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        if build_if_missing:
            from . import _build
            _build.build()
        else:
            raise RuntimeError("libaigar_hip.so not found at %s: build it with `python -m aigar_amd._build` "
                               "(hipcc --offload-arch=gfx950)" % SO_PATH)
    _preload_single_hip_runtime()
    L = C.CDLL(SO_PATH)
    vp, i32, u64, dp = C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_double)
    L.aigar_last_error.restype = C.c_char_p
    L.aigar_abi_version.restype = i32
    sig = {
        "aigar_create": [C.POINTER(_abi.Config), C.POINTER(vp)],
        "aigar_destroy": [vp],
        "aigar_reset": [vp, u64],
        "aigar_reset_arenas": [vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), i32],
        "aigar_set_commands": [vp, vp, i32],
        "aigar_policy_random": [vp, C.c_double, C.c_double, u64],
        "aigar_step": [vp, i32],
        "aigar_obs_len": [vp],
        "aigar_observe": [vp, vp, i32, i32],
        "aigar_observe_pixels": [vp, vp, i32, u64, i32, i32],
        "aigar_pixel_config": [vp, C.POINTER(_abi.PixelParams)],
        "aigar_pixel_state_len": [vp],
        "aigar_observe_pixel_state": [vp, vp, i32, i32, vp, i32],
        "aigar_exp_config": [vp, C.POINTER(_abi.ExpParams)],
        "aigar_exp_info": [vp, C.POINTER(C.c_int64)],
        "aigar_exp_add": [vp, vp, vp, vp, vp, vp, vp, i32, i32],
        "aigar_exp_sample": [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp],
        "aigar_exp_gather": [vp, vp, i32, vp, vp, vp, vp, vp],
        "aigar_exp_update_priorities": [vp, vp, vp, i32],
        "aigar_decide_config": [vp, C.POINTER(_abi.DecideParams), vp],
        "aigar_decide": [vp, vp, vp, vp, vp, vp, vp],
        "aigar_env_step_q": [vp, vp, vp, vp, i32, i32, C.POINTER(_abi.RewardParams), vp, vp, i32, vp, vp],
        "aigar_noise_config": [vp, C.POINTER(_abi.NoiseParams)],
        "aigar_noise": [vp, vp, i32, vp, vp, i32, vp, vp, vp],
        "aigar_env_step_ac": [vp, vp, vp, vp, i32, i32, i32, C.POINTER(_abi.RewardParams), vp, vp, i32, vp],
        "aigar_net_config": [vp, C.POINTER(_abi.NetParams)],
        "aigar_net_set_weights": [vp, i32, vp, vp, i32],
        "aigar_net_forward": [vp, vp, i32, i32, vp],
        "aigar_net_output": [vp, vp],
        "aigar_net_config_cnn": [vp, C.POINTER(_abi.ConvParams), C.POINTER(_abi.NetParams)],
        "aigar_net_set_conv_weights": [vp, i32, vp, vp, i32],
        "aigar_env_step_net": [vp, i32, vp, vp, i32, i32, i32, C.POINTER(_abi.RewardParams), vp, vp, i32, vp, vp, vp,
                               i32],
        "aigar_train_config": [vp, C.POINTER(_abi.TrainParams)],
        "aigar_train_step": [vp, i32, vp],
        "aigar_train_info": [vp, C.POINTER(C.c_int64)],
        "aigar_train_td": [vp, vp, vp],
        "aigar_train_sync_target": [vp],
        "aigar_train_reset": [vp],
        "aigar_critic_config": [vp, C.POINTER(_abi.NetParams)],
        "aigar_critic_set_weights": [vp, i32, vp, vp, i32],
        "aigar_critic_forward": [vp, vp, i32, i32, vp],
        "aigar_actrain_config": [vp, C.POINTER(_abi.ActrainParams)],
        "aigar_actrain_step": [vp, i32, vp],
        "aigar_actrain_info": [vp, C.POINTER(C.c_int64)],
        "aigar_actrain_td": [vp, vp, vp, vp],
        "aigar_actrain_var": [vp, C.POINTER(C.c_double)],
        "aigar_actrain_sync_target": [vp],
        "aigar_actrain_reset": [vp],
        "aigar_qcritic_config": [vp, C.POINTER(_abi.NetParams)],
        "aigar_dpg_config": [vp, C.POINTER(_abi.DpgParams)],
        "aigar_dpg_step": [vp, i32, vp],
        "aigar_dpg_info": [vp, C.POINTER(C.c_int64)],
        "aigar_dpg_td": [vp, vp, vp],
        "aigar_dpg_sync_target": [vp],
        "aigar_dpg_reset": [vp],
        "aigar_spg_config": [vp, C.POINTER(_abi.SpgParams)],
        "aigar_spg_step": [vp, i32, vp, vp],
        "aigar_spg_info": [vp, C.POINTER(C.c_int64)],
        "aigar_spg_td": [vp, vp, vp],
        "aigar_spg_noise": [vp, C.POINTER(vp)],
        "aigar_spg_sync_target": [vp],
        "aigar_spg_reset": [vp],
        "aigar_net_get_weights": [vp, i32, i32, vp, vp, i32],
        "aigar_net_pad_check": [vp, i32, C.POINTER(C.c_int64)],
        "aigar_train_config_cnn": [vp, C.POINTER(_abi.TrainParams)],
        "aigar_net_get_conv_weights": [vp, i32, i32, vp, vp, i32],
        "aigar_exp_extra_get": [vp, vp, i32, vp, vp],
        "aigar_exp_extra_set": [vp, vp, vp, i32],
        "aigar_warnings": [vp, i32, C.POINTER(C.c_uint32)],
        "aigar_set_actions": [vp, vp, vp, i32],
        "aigar_reset_bots": [vp, vp, i32],
        "aigar_player_stats": [vp, vp, i32],
        "aigar_score": [vp, vp, i32],
        "aigar_score_reset": [vp, vp, i32],
        "aigar_score_trace": [vp, vp, C.c_int64],
        "aigar_get_state": [vp, i32, C.POINTER(_abi.State)],
        "aigar_load_state": [vp, i32, C.POINTER(_abi.State)],
        "aigar_get_events": [vp, i32, C.POINTER(C.c_int64), i32, C.POINTER(i32)],
        "aigar_set_stream": [vp, vp],
        "aigar_sync": [vp],
        "aigar_profile": [vp, i32],
        "aigar_kernel_time": [vp, C.c_char_p, dp, C.POINTER(i32)],
        "aigar_selftest_pow": [dp, dp, dp, i32],
        "aigar_selftest_log": [dp, dp, i32],
        "aigar_selftest_trig": [dp, dp, dp, i32],
        "aigar_selftest_sem": [i32, dp, i32, dp, i32, i32],
        "aigar_counters": [vp, i32, C.POINTER(C.c_int64), i32],
        "aigar_policy_greedy": [vp, i32, vp, i32],
        "aigar_apply_actions": [vp, vp, i32, i32, i32, i32, i32],
        "aigar_rewards": [vp, vp, C.POINTER(_abi.RewardParams), i32, i32],
        "aigar_set_split_likelihood": [vp, i32, C.POINTER(C.c_int32)],
        "aigar_run": [vp, i32, C.POINTER(_abi.RunParams), vp, i32],
        "aigar_env_step": [vp, vp, i32, i32, i32, C.POINTER(_abi.RewardParams), vp, vp, i32],
        "aigar_get_events_raw": [vp, i32, C.POINTER(C.c_int64), i32, C.POINTER(i32)],
        "aigar_observe_masked": [vp, vp, i32, i32, vp, i32],
        "aigar_set_roles": [vp, vp, i32],
        "aigar_env_config": [vp, C.POINTER(_abi.EnvParams)],
        "aigar_policy_random_bots": [vp],
        "aigar_tile_info": [vp, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)],
        "aigar_tile_set_buffers": [vp, vp, vp],
        "aigar_tile_msg_bytes": [vp, C.POINTER(C.c_int64)],
        "aigar_tile_begin": [vp, C.POINTER(_abi.RunParams)],
        "aigar_tile_policy": [vp, i32],
        "aigar_tile_apply_commands": [vp],
        "aigar_tile_apply": [vp, C.POINTER(i32)],
        "aigar_tile_resume": [vp],
        "aigar_tile_end": [vp, vp, i32],
        "aigar_tile_exchange_local": [C.POINTER(vp), i32],
        "aigar_tile_observers": [vp, C.POINTER(C.c_int32)],
        "aigar_rccl_unique_id": [C.c_char_p, vp],
        "aigar_tile_comm_init": [vp, C.c_char_p, vp, i32, i32],
        "aigar_tile_run": [vp, i32, C.POINTER(_abi.RunParams), i32, vp, i32],
        "aigar_tile_run_graphed": [vp],
        "aigar_tile_loopback": [vp],
    }
    for name, args in sig.items():
        f = getattr(L, name, None)
        if f is None and os.environ.get("AIGAR_SO"):  # an older diagnostics build: bind what it has
            continue
        if f is None:
            raise RuntimeError("libaigar_hip.so lacks %s: rebuild it (python -m aigar_amd._build)" % name)
        f.argtypes = args
        f.restype = i32
    if L.aigar_abi_version() != _abi.ABI_VERSION:
        raise RuntimeError("libaigar_hip.so ABI %d != python binding %d" % (L.aigar_abi_version(), _abi.ABI_VERSION))
    _lib = L
    return L


def _ptr(x):
    """Host numpy array or device tensor -> (void pointer, on_device)."""
    if x is None:
        return None, 0
    if isinstance(x, np.ndarray):
        return x.ctypes.data_as(C.c_void_p), 0
    if hasattr(x, "data_ptr"):  # torch tensor (device memory when x.is_cuda)
        return C.c_void_p(x.data_ptr()), int(bool(getattr(x, "is_cuda", False)))
    raise TypeError("expected numpy array or torch tensor, got %r" % type(x))


_DTYPE_NAMES = {}  # dtype -> its bare name (every checked tensor of every call asks: the strings are made once)


def _dtype_name(dtype, what=None):
    """A numpy / torch dtype (or its name) -> the bare name, "float64" for torch.float64 and
    for numpy.float64.  what: the caller and its argument ("net_config: x_dtype"), for a value
    that must be float64 or float32 -- anything else is refused under that name."""
    try:
        d = _DTYPE_NAMES[dtype]
    except KeyError:
        d = _DTYPE_NAMES[dtype] = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
    if what is not None and d not in ("float64", "float32"):
        raise ValueError("%s must be float64 or float32, got %s" % (what, dtype))
    return d


def _dtype_code(d):
    """The library's code of a floating dtype name: 0 float64, 1 float32."""
    return 0 if d == "float64" else 1


def _reward_params(params):
    """A parameters object (or None: the defaults) -> _abi.RewardParams; one is passed through."""
    return params if isinstance(params, _abi.RewardParams) else _abi.RewardParams.from_parameters(params)


class Stepper:
    """One handle of the device stepper: n_arenas fields x bots_per_arena players."""

    def __init__(self, cfg):
        self.L = load()
        self.cfg = cfg
        h = C.c_void_p()
        self._chk(self.L.aigar_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.A, self.B = cfg.n_arenas, cfg.bots_per_arena
        self.NP = self.A * self.B
        self.obs_len = self.L.aigar_obs_len(self.h)
        self.pixel_state_shape = None  # (NP, side, side, C) while a pixel state is configured
        self.exp = None  # (state row shape, state dtype name, prioritized) while a replay memory is configured
        self.dec = None  # (n_out, q dtype name) while an action selection is configured
        self.noi = None  # (n_act, mu dtype name, Orn-Uhl) while an exploration noise is configured
        self.net = None  # (n_in, units, state dtype name) while an acting network is configured
        self.conv = None  # (side, channels, convs) while that network has a conv part (n_in: the flattened length)
        self.trn = None  # the batch while a training is configured
        self.crit = None  # (n_in, units) while a critic is configured
        self.act = None  # the batch while a CACLA training is configured
        self.dpg = None  # the batch while a DPG training is configured
        self.spg = None  # (batch, samples) while an SPG training is configured

    def _chk(self, r):
        if r < 0:
            raise RuntimeError("aigar: " + self.L.aigar_last_error().decode())
        return r

    def close(self):
        if getattr(self, "h", None):
            self.L.aigar_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, seed=0):
        self._chk(self.L.aigar_reset(self.h, int(seed)))

    def set_commands(self, cmd):
        if isinstance(cmd, np.ndarray):
            cmd = np.ascontiguousarray(cmd, np.float64).reshape(self.NP, 4)
        p, dev = _ptr(cmd)
        self._chk(self.L.aigar_set_commands(self.h, p, dev))

    def policy_random(self, p_split=0.0, p_eject=0.0, seed=0):
        self._chk(self.L.aigar_policy_random(self.h, float(p_split), float(p_eject), int(seed)))

    def _mask_ptr(self, mask):
        """A per-player mask (None: everybody) -> (void pointer, on_device): a numpy array
        becomes the [NP] uint8 the library reads, a device tensor goes as it is."""
        if isinstance(mask, np.ndarray):
            mask = np.ascontiguousarray(mask, np.uint8).reshape(self.NP)
        return _ptr(mask)

    def policy_greedy(self, greedy_split=False, mask=None):
        """Greedy bots' moves (bot.py:579-633) for the players where mask != 0 (all if None)."""
        p, dev = self._mask_ptr(mask)
        self._chk(self.L.aigar_policy_greedy(self.h, int(bool(greedy_split)), p, dev))

    def apply_actions(self, act, enable_split=True, skipping=False, record=True):
        """Learner actions act[NP, n] (n = 2..4, numpy or device tensor) through set_command_point."""
        if isinstance(act, np.ndarray):
            act = np.ascontiguousarray(act, np.float64).reshape(self.NP, -1)
        n = int(act.shape[1])
        p, dev = _ptr(act)
        self._chk(self.L.aigar_apply_actions(self.h, p, n, int(bool(enable_split)), int(bool(skipping)),
                                             int(bool(record)), dev))

    def rewards(self, params=None, update_last=True, out=None):
        """Bot.getReward for every player (NaN where the reference has None)."""
        prm = _reward_params(params)
        if out is None:
            out = np.zeros(self.NP, np.float64)
        p, dev = _ptr(out)
        self._chk(self.L.aigar_rewards(self.h, p, C.byref(prm), int(bool(update_last)), dev))
        return out

    def set_split_likelihood(self, lh, arena=0):
        if lh is None:
            self._chk(self.L.aigar_set_split_likelihood(self.h, arena, None))
            return
        a = np.ascontiguousarray(lh, np.int32).reshape(self.B)
        self._chk(self.L.aigar_set_split_likelihood(self.h, arena, a.ctypes.data_as(C.POINTER(C.c_int32))))

    def step(self, n=1):
        self._chk(self.L.aigar_step(self.h, int(n)))

    def run(self, n, policy="random", out=None, p_split=0.0, p_eject=0.0, seed=0, greedy_split=False):
        """n whole env steps (policy + Field.update + observation into the DEVICE tensor out,
        or no observation when out is None), replayed from one captured hipGraph."""
        pol = {"none": _abi.POLICY_NONE, "random": _abi.POLICY_RANDOM, "greedy": _abi.POLICY_GREEDY}[policy]
        prm = _abi.RunParams(pol, int(bool(greedy_split)), float(p_split), float(p_eject), int(seed))
        p, dt = None, 0
        if out is not None:
            if not getattr(out, "is_cuda", False):
                raise ValueError("aigar_run writes observations to a device tensor")
            dt = _dtype_code(_dtype_name(out.dtype))
            if tuple(out.shape) != (self.NP, self.obs_len):
                raise ValueError("observation tensor must be [%d, %d]" % (self.NP, self.obs_len))
            p = C.c_void_p(out.data_ptr())
        self._chk(self.L.aigar_run(self.h, int(n), C.byref(prm), p, dt))
        return out

    def env_step(self, act, reward, obs, enable_split=True, skip=0, params=None):
        """One learner decision on device tensors (aigar_env_step): act [NP, 2..4] float64,
        reward [NP] float64 (summed over the skip + 1 ticks), obs [NP, obs_len]; one graph replay."""
        for t in (act, reward, obs):
            if not getattr(t, "is_cuda", False) or not t.is_contiguous():
                raise ValueError("env_step takes contiguous device tensors")
        if str(act.dtype) != "torch.float64" or str(reward.dtype) != "torch.float64":
            raise ValueError("actions and rewards are float64")
        if act.dim() != 2 or act.shape[0] != self.NP or not 2 <= act.shape[1] <= 4:
            raise ValueError("actions must be [%d, 2..4]" % self.NP)
        if self.pixel_state_shape is not None:
            if tuple(reward.shape) != (self.NP,):
                raise ValueError("reward must be [%d]" % self.NP)
        elif tuple(obs.shape) != (self.NP, self.obs_len) or tuple(reward.shape) != (self.NP,):
            raise ValueError("reward must be [%d], obs [%d, %d]" % (self.NP, self.NP, self.obs_len))
        prm, rp, op, dt = self._decision_tail("env_step", reward, obs, params)
        self._chk(self.L.aigar_env_step(self.h, C.c_void_p(act.data_ptr()), int(act.shape[1]), int(bool(enable_split)),
                                        int(skip), prm, rp, op, dt))

    def _decision_tail(self, what, reward, obs, params, pixels=True):
        """What every decision call ends with: reward [NP] float64 and obs, the handle's states
        (the pixel state while one is configured and pixels holds, else the grid row) in float64
        or float32, both contiguous device tensors; params as rewards() takes them.  Returns the
        call's RewardParams pointer, the two tensors' pointers and obs' dtype code."""
        for t in (reward, obs):
            if not getattr(t, "is_cuda", False) or not t.is_contiguous():
                raise ValueError("%s takes contiguous device tensors" % what)
        rp = self._dev_ptr(reward, (self.NP,), ("float64",), what)
        shape = self.pixel_state_shape if pixels and self.pixel_state_shape is not None else (self.NP, self.obs_len)
        d = self._check_out(obs, shape, ("float64", "float32"), what)
        return C.byref(_reward_params(params)), rp, C.c_void_p(obs.data_ptr()), _dtype_code(d)

    def _check_out(self, out, shape, dtypes, what):
        """The library writes prod(shape) elements of the dtype into out: refuse a
        buffer of another shape / dtype, a strided view or a tensor on another device."""
        d = _dtype_name(getattr(out, "dtype", ""))
        if tuple(out.shape) != tuple(shape):
            raise ValueError("%s: out must have shape %s, got %s" % (what, tuple(shape), tuple(out.shape)))
        if d not in dtypes:
            raise ValueError("%s: out dtype must be one of %s, got %s" % (what, dtypes, d))
        contig = out.flags["C_CONTIGUOUS"] if isinstance(out, np.ndarray) else out.is_contiguous()
        if not contig:
            raise ValueError("%s: out must be C-contiguous" % what)
        if hasattr(out, "is_cuda") and out.is_cuda and out.device.index not in (None, self.cfg.device):
            raise ValueError("%s: out is on cuda:%s, the stepper on device %d" % (what, out.device.index,
                                                                                 self.cfg.device))
        return d

    def observe(self, out=None, dtype=np.float64, mask=None):
        """getStateRepresentation of every player (mask: only where mask != 0; the
        other rows of out are kept and those bots' history does not advance)."""
        if out is None:
            out = np.zeros((self.NP, self.obs_len), dtype)
        d = self._check_out(out, (self.NP, self.obs_len), ("float64", "float32"), "observe")
        dt = _dtype_code(d)
        p, dev = _ptr(out)
        if mask is None:
            self._chk(self.L.aigar_observe(self.h, p, dt, dev))
        else:
            mp, mdev = self._mask_ptr(mask)
            self._chk(self.L.aigar_observe_masked(self.h, p, dt, dev, mp, mdev))
        return out

    def set_roles(self, roles):
        """Player roles of a mixed population: AIGAR_ROLE_* codes or "NN" / "Greedy" / "Random"."""
        r = np.array([_abi.ROLES.get(x, x) if isinstance(x, str) else x for x in roles], np.uint8).reshape(self.NP)
        self._chk(self.L.aigar_set_roles(self.h, r.ctypes.data_as(C.c_void_p), 0))

    def env_config(self, greedy_split=False, random_skip=7, random_split=False, random_eject=False, salt=0):
        prm = _abi.EnvParams(int(bool(greedy_split)), int(random_skip), int(bool(random_split)),
                             int(bool(random_eject)), int(salt))
        self._chk(self.L.aigar_env_config(self.h, C.byref(prm)))

    def policy_random_bots(self):
        self._chk(self.L.aigar_policy_random_bots(self.h))

    def reset_arenas(self, arenas, seeds):
        """Field.reset of the listed (distinct) arenas, arena arenas[k] becoming the world a
        one-arena handle gets from reset(seeds[k]); their bots reset as by load_state, the
        other arenas untouched.  Kernels on the stepper's stream: no host round trip."""
        a = np.ascontiguousarray(arenas, np.int32).reshape(-1)
        s = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], np.uint64).reshape(-1)
        if len(a) != len(s):
            raise ValueError("reset_arenas: %d arenas, %d seeds" % (len(a), len(s)))
        self._chk(self.L.aigar_reset_arenas(self.h, a.ctypes.data_as(C.POINTER(C.c_int32)),
                                            s.ctypes.data_as(C.POINTER(C.c_uint64)), len(a)))

    def reset_arena(self, arena, seed):
        """reset_arenas for ONE arena (for n_arenas == 1: the world of reset(seed))."""
        self.reset_arenas([arena], [seed])

    def observe_pixels(self, side=42, color_seed=0, rgb=True, out=None):
        """RGBGenerator.get_cnn_inputRGB for every player (rgbGenerator.py:95-110):
        uint8 [NP, side, side, 3] when rgb, else float64/float32 grayscale [NP, side, side]."""
        if out is None:
            out = np.zeros((self.NP, side, side, 3), np.uint8) if rgb else np.zeros((self.NP, side, side), np.float64)
        d = _dtype_name(getattr(out, "dtype", ""))
        if d == "uint8":
            self._check_out(out, (self.NP, side, side, 3), ("uint8",), "observe_pixels")
        else:
            self._check_out(out, (self.NP, side, side), ("float64", "float32"), "observe_pixels")
        dt = 2 if d == "uint8" else _dtype_code(d)
        p, dev = _ptr(out)
        self._chk(self.L.aigar_observe_pixels(self.h, p, int(side), int(color_seed), dt, dev))
        return out

    def pixel_config(self, side, rgb=False, last=False, color_seed=0):
        """The learner's pixel state (CNN_P_REPR, bot.py:276-282): side x side frames of
        1 (grayscale) or 3 (rgb) channels through (frame - 255) / 100, doubled by last
        ([current | the bot's previous frame]).  While it is set, env_step writes it instead
        of the grid row.  pixel_config(None) turns it off.  Clears the frame history."""
        if side is None:
            self._chk(self.L.aigar_pixel_config(self.h, None))
            self.pixel_state_shape = None
            return
        prm = _abi.PixelParams(int(side), (_abi.PIX_RGB if rgb else 0) | (_abi.PIX_LAST if last else 0),
                               int(color_seed) & 0xFFFFFFFFFFFFFFFF)
        self._chk(self.L.aigar_pixel_config(self.h, C.byref(prm)))
        n = self.L.aigar_pixel_state_len(self.h)
        self.pixel_state_shape = (self.NP, int(side), int(side), n // (int(side) * int(side)))

    def observe_pixel_state(self, out=None, dtype=np.float32, mask=None):
        """The configured pixel state of every player, [NP, side, side, C] float64 / float32
        (mask: only where mask != 0; the other rows of out are kept and those bots' frame
        history does not advance).  Dead players: NaN rows."""
        if self.pixel_state_shape is None:
            raise RuntimeError("aigar: observe_pixel_state: no pixel state is configured (pixel_config)")
        if out is None:
            out = np.zeros(self.pixel_state_shape, dtype)
        d = self._check_out(out, self.pixel_state_shape, ("float64", "float32"), "observe_pixel_state")
        p, dev = _ptr(out)
        mp, mdev = self._mask_ptr(mask)
        self._chk(self.L.aigar_observe_pixel_state(self.h, p, _dtype_code(d), dev, mp, mdev))
        return out

    # ---- replay memory (include/aigar.h: aigar_exp_*)
    def exp_config(self, capacity, prioritized=False, alpha=0.6, beta=0.4, dtype="float64", seed=0, extra=False):
        """The handle's replay memory (replay_buffer.py): a ring of capacity transitions whose
        states have the handle's current state shape (the pixel state when one is configured,
        else the observation row) in dtype; prioritized: with the sum / min trees.  While it
        is set every env_step appends the NN players' transitions inside its graph.  extra:
        the ring also keeps the tuple's fifth field (exp_extra_get / exp_extra_set).
        exp_config(None) frees it."""
        self.trn = self.act = self.dpg = self.spg = None  # (the library drops the train configurations with the memory)
        if not capacity:
            self._chk(self.L.aigar_exp_config(self.h, None))
            self.exp = None
            return
        d = _dtype_name(dtype, "exp_config: dtype")
        flags = (_abi.EXP_PRIORITIZED if prioritized else 0) | (_abi.EXP_EXTRA if extra else 0)
        prm = _abi.ExpParams(int(capacity), _dtype_code(d), flags, float(alpha), float(beta),
                             int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._chk(self.L.aigar_exp_config(self.h, C.byref(prm)))
        row = tuple(self.pixel_state_shape[1:]) if self.pixel_state_shape is not None else (self.obs_len,)
        self.exp = (row, d, bool(prioritized))

    def _need_exp(self, what):
        if self.exp is None:
            raise RuntimeError("aigar: %s: no replay memory is configured (exp_config)" % what)
        return self.exp

    def _dev_ptr(self, t, shape, dtypes, what, optional=False):
        """The pointer of a device tensor the library reads or writes as prod(shape) elements of
        one of dtypes (optional: None for None): anything _check_out refuses, and what is no
        tensor on a device, is refused under the caller's name."""
        if t is None and optional:
            return None
        if not getattr(t, "is_cuda", False):
            raise ValueError("%s takes device tensors" % what)
        self._check_out(t, shape, dtypes, what)
        return C.c_void_p(t.data_ptr())

    def exp_info(self):
        """{capacity, size, next_idx, added} of the memory (a host round trip)."""
        self._need_exp("exp_info")
        v = (C.c_int64 * 4)()
        self._chk(self.L.aigar_exp_info(self.h, v))
        return {"capacity": v[0], "size": v[1], "next_idx": v[2], "added": v[3]}

    def exp_add(self, s, a, r, s2, done, mask=None):
        """ReplayBuffer.add for the rows with mask != 0 (all if None), in row order: s, s2
        [n, *state shape] of the memory's dtype, a [n, 4] and r [n] float64, done [n] uint8 /
        bool; all numpy arrays or all device tensors."""
        row, d, _ = self._need_exp("exp_add")
        n = int(s.shape[0])
        dev = None
        ptrs = []
        for x, shape, dts in ((s, (n,) + row, (d,)), (a, (n, 4), ("float64",)), (r, (n,), ("float64",)),
                              (s2, (n,) + row, (d,)), (done, (n,), ("uint8", "bool")),
                              (mask, (n,), ("uint8", "bool"))):
            if x is None:
                ptrs.append(None)
                continue
            self._check_out(x, shape, dts, "exp_add")
            p, on = _ptr(x)
            if dev is not None and on != dev:
                raise ValueError("exp_add: all numpy arrays or all device tensors")
            dev = on
            ptrs.append(p)
        self._chk(self.L.aigar_exp_add(self.h, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], n, dev))

    def _exp_rows(self, batch, s, a, r, s2, done, what):
        row, d, _ = self._need_exp(what)
        args = ((s, (batch,) + row, (d,)), (a, (batch, 4), ("float64",)), (r, (batch,), ("float64",)),
                (s2, (batch,) + row, (d,)), (done, (batch,), ("uint8", "bool")))
        return [self._dev_ptr(x, shape, dts, what, optional=True) for x, shape, dts in args]

    def exp_sample(self, w, idx, u=None, s=None, a=None, r=None, s2=None, done=None):
        """One mini-batch of len(idx) draws on device tensors (aigar_exp_sample): idx [batch]
        int64 and w [batch] float64 are written, and row k of the given s, a, r, s2, done
        gets transition idx[k]; u [batch] float64 in [0, 1) are the draws (None: the
        memory's own Philox stream).  Stream-ordered, no host round trip."""
        batch = int(idx.shape[0])
        rows = self._exp_rows(batch, s, a, r, s2, done, "exp_sample")
        wp = self._dev_ptr(w, (batch,), ("float64",), "exp_sample")
        ip = self._dev_ptr(idx, (batch,), ("int64",), "exp_sample")
        up = self._dev_ptr(u, (batch,), ("float64",), "exp_sample", optional=True)
        self._chk(self.L.aigar_exp_sample(self.h, batch, up, rows[0], rows[1], rows[2], rows[3], rows[4], wp, ip))

    def exp_gather(self, idx, s=None, a=None, r=None, s2=None, done=None):
        """Row k of the given device tensors gets transition idx[k] (idx: int64 device tensor);
        rows whose index is outside [0, size) are left as they are."""
        batch = int(idx.shape[0])
        rows = self._exp_rows(batch, s, a, r, s2, done, "exp_gather")
        ip = self._dev_ptr(idx, (batch,), ("int64",), "exp_gather")
        self._chk(self.L.aigar_exp_gather(self.h, ip, batch, *rows))

    def exp_update_priorities(self, idx, prio):
        """PrioritizedReplayBuffer.update_priorities on device tensors idx [n] int64, prio [n]
        float64 (the last of a repeated index wins; prio <= 0 and indices outside [0, size)
        are skipped); nothing in uniform mode."""
        self._need_exp("exp_update_priorities")
        n = int(idx.shape[0])
        ip = self._dev_ptr(idx, (n,), ("int64",), "exp_update_priorities")
        pp = self._dev_ptr(prio, (n,), ("float64",), "exp_update_priorities")
        self._chk(self.L.aigar_exp_update_priorities(self.h, ip, pp, n))

    def exp_extra_get(self, idx, out=None, valid=None):
        """The fifth field of the slots idx [batch] (int64 device tensor) into the device tensors
        out [batch, 4] float64 and valid [batch] uint8 / bool; rows whose index is outside
        [0, size) are left as they are.  The memory needs extra=True."""
        self._need_exp("exp_extra_get")
        batch = int(idx.shape[0])
        ip = self._dev_ptr(idx, (batch,), ("int64",), "exp_extra_get")
        op = self._dev_ptr(out, (batch, 4), ("float64",), "exp_extra_get", optional=True)
        vp = self._dev_ptr(valid, (batch,), ("uint8", "bool"), "exp_extra_get", optional=True)
        self._chk(self.L.aigar_exp_extra_get(self.h, ip, batch, op, vp))

    def exp_extra_set(self, idx, rows):
        """ReplayBuffer.update_dones on device tensors idx [n] int64, rows [n, 4] float64: slot
        idx[j] gets rows[j] and becomes valid (the last of a repeated index wins; indices
        outside [0, size) are skipped).  The memory needs extra=True."""
        self._need_exp("exp_extra_set")
        n = int(idx.shape[0])
        ip = self._dev_ptr(idx, (n,), ("int64",), "exp_extra_set")
        rp = self._dev_ptr(rows, (n, 4), ("float64",), "exp_extra_set")
        self._chk(self.L.aigar_exp_extra_set(self.h, ip, rp, n))

    # ---- exploration noise of the actor-critic learners (include/aigar.h: aigar_noise*)
    def noise_config(self, n_act, kind="Gaussian", mu_dtype="float32", theta=0.15, ou_mu=0.0, dt=0.01, seed=0,
                     store_raw=False):
        """The handle's exploration noise (actorCritic.py:922-936): n_act values per action
        (2..4), kind "Gaussian" or "Orn-Uhl" (or its code), mu_dtype the dtype of the actor's
        rows, theta / ou_mu / dt the Orn-Uhl parameters, seed the salt of the own draws,
        store_raw: the replay memory's extra field gets the raw action (CACLA).
        noise_config(None) turns it off."""
        if n_act is None:
            self._chk(self.L.aigar_noise_config(self.h, None))
            self.noi = None
            return
        d = _dtype_name(mu_dtype, "noise_config: mu_dtype")
        k = _abi.NOISE_TYPES[kind] if isinstance(kind, str) else int(kind)
        prm = _abi.NoiseParams(int(n_act), k, _dtype_code(d), int(bool(store_raw)), float(theta),
                               float(ou_mu), float(dt), int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._chk(self.L.aigar_noise_config(self.h, C.byref(prm)))
        self.noi = (int(n_act), d, k == _abi.NOISE_ORN_UHL)

    def _noise_args(self, mu, rows, std, u, what):
        if self.noi is None:
            raise RuntimeError("aigar: %s: no exploration noise is configured (noise_config)" % what)
        n, d, _ = self.noi
        mp = self._dev_ptr(mu, (rows, n), (d,), what)
        sp = self._dev_ptr(std, (1,), ("float64",), what)
        return (mp, sp) + self._draws_arg(u, rows, "rows", what)

    def _draws_arg(self, u, rows, rows_name, what):
        """The noise's draws u [rows, 2, T, 2] float64 -> (pointer, T); (None, 0) for None, the
        own Philox stream.  rows_name: how the caller's message calls the first dimension."""
        if u is None:
            return None, 0
        if u.dim() != 4 or not 1 <= int(u.shape[2]) <= _abi.NOISE_MAX_T:
            raise ValueError("%s: u must be [%s, 2, T, 2] with T in 1..%d" % (what, rows_name, _abi.NOISE_MAX_T))
        T = int(u.shape[2])
        return self._dev_ptr(u, (rows, 2, T, 2), ("float64",), what), T

    def noise(self, mu, std, out, u=None, prev=None, n_exhausted=None):
        """The perturbation alone on device tensors (aigar_noise): mu [rows, n_act], std [1]
        float64, u [rows, 2, T, 2] float64 uniforms in [0, 1) (None: the own Philox stream),
        prev [rows, n_act] float64 the caller's Orn-Uhl state (advanced in place), n_exhausted
        [1] int64 counter of exhausted pairs; writes out [rows, n_act] float64.  Liveness and
        roles are ignored."""
        rows = int(mu.shape[0])
        mp, sp, up, T = self._noise_args(mu, rows, std, u, "noise")
        n = self.noi[0]
        op = self._dev_ptr(out, (rows, n), ("float64",), "noise")
        pp = self._dev_ptr(prev, (rows, n), ("float64",), "noise", optional=True)
        ep = self._dev_ptr(n_exhausted, (1,), ("int64",), "noise", optional=True)
        self._chk(self.L.aigar_noise(self.h, mp, rows, sp, up, T, pp, op, ep))

    def env_step_ac(self, mu, std, reward, obs, u=None, noisy=None, enable_split=True, skip=0, params=None):
        """One actor-critic decision on device tensors (aigar_env_step_ac): the noise, then
        env_step with the noisy rows; one graph replay.  noisy [NP, n_act] float64 gets the
        noisy actions (NaN rows where nobody decided)."""
        mp, sp, up, T = self._noise_args(mu, self.NP, std, u, "env_step_ac")
        prm, rp, op, dt = self._decision_tail("env_step_ac", reward, obs, params)
        np_ = self._dev_ptr(noisy, (self.NP, self.noi[0]), ("float64",), "env_step_ac", optional=True)
        self._chk(self.L.aigar_env_step_ac(self.h, mp, sp, up, T, int(bool(enable_split)), int(skip), prm, rp, op, dt,
                                           np_))

    @staticmethod
    def selftest_log(x):
        """Device log (glibc's, restated in aigar_math.h) for a host array."""
        return selftest_log(x)

    # ---- what the acting network and the critic share: each is a stack of dense layers of the handle
    _NET_CODES = {"online": _abi.NET_ONLINE, "target": _abi.NET_TARGET, "m": _abi.NET_ADAM_M, "v": _abi.NET_ADAM_V}
    _CRITIC_CODES = {"online": _abi.NET_CRITIC, "target": _abi.NET_CRITIC_TARGET, "m": _abi.NET_CRITIC_M,
                     "v": _abi.NET_CRITIC_V}

    def _dense_params(self, what, n_in, units, hidden, out, x_dtype, min_layers):
        """The NetParams of a dense stack -> (params, units, state dtype name): the activations by
        name or code, x_dtype a numpy or torch dtype or its name; another dtype and a layer count
        outside min_layers..NET_MAX_LAYERS are refused under the caller's name."""
        units = [int(v) for v in units]
        d = _dtype_name(x_dtype, what + ": x_dtype")
        if not min_layers <= len(units) <= 8:
            raise ValueError("%s: %d layers, %s%d" % (what, len(units), "1.." if min_layers else "at most ",
                                                      _abi.NET_MAX_LAYERS))
        code = lambda a: _abi.ACTIVATIONS[a] if isinstance(a, str) else int(a)
        prm = _abi.NetParams(len(units), int(n_in), _dtype_code(d), code(hidden), code(out), 0)
        for i, v in enumerate(units):
            prm.units[i] = v
        return prm, tuple(units), d

    def _push_pair(self, what, push, l, W, b, shape):
        """Layer l's weights through push (an aigar_*_set_*weights entry): W of shape and b
        [shape[-1]], float32, both numpy arrays (anything else is made one) or both device tensors."""
        if isinstance(W, np.ndarray) or not hasattr(W, "data_ptr"):
            W, b = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(b, np.float32)
        self._check_out(W, shape, ("float32",), what)
        self._check_out(b, (shape[-1],), ("float32",), what)
        (wp, on), (bp, on_b) = _ptr(W), _ptr(b)
        if on != on_b:
            raise ValueError("%s: W and b both numpy arrays or both device tensors" % what)
        self._chk(push(self.h, l, wp, bp, on))

    def _push_dense(self, what, push, n_in, units, weights):
        for l, (W, b) in enumerate(weights):
            self._push_pair(what, push, l, W, b, (units[l - 1] if l else n_in, units[l]))

    def _read_dense(self, what, codes, which, n_in, units, device=False):
        """[(W [in, out], b [out])] float32 of the stack's copy codes[which] (aigar_net_get_weights)."""
        if which not in codes:
            raise ValueError("%s: which must be one of %s" % (what, sorted(codes)))
        out = []
        for l, n in enumerate(units):
            k = units[l - 1] if l else n_in
            if device:
                import torch
                dev = "cuda:%d" % self.cfg.device
                W = torch.empty((k, n), dtype=torch.float32, device=dev)
                b = torch.empty((n,), dtype=torch.float32, device=dev)
            else:
                W, b = np.empty((k, n), np.float32), np.empty((n,), np.float32)
            self._chk(self.L.aigar_net_get_weights(self.h, codes[which], l, _ptr(W)[0], _ptr(b)[0], int(device)))
            out.append((W, b))
        return out

    def _pad_check(self, codes, which):
        v = C.c_int64()
        self._chk(self.L.aigar_net_pad_check(self.h, codes[which], C.byref(v)))
        return int(v.value)

    def _forward(self, what, forward, x, xshape, out, oshape):
        """x of xshape, float64 / float32, through forward (an aigar_*_forward entry) into out of
        oshape, float64; rows is the first dimension of both."""
        xp = self._dev_ptr(x, xshape, ("float64", "float32"), what)
        op = self._dev_ptr(out, oshape, ("float64",), what)
        self._chk(forward(self.h, xp, _dtype_code(_dtype_name(x.dtype)), xshape[0], op))

    # ---- the learners' acting network (include/aigar.h: aigar_net*)
    def net_config(self, spec, x_dtype="float64"):
        """The handle's acting network: spec is (n_in, units, hidden, out) -- the state
        length, the outputs of every dense layer, and the activations by name or code
        (aigar_amd.net.mlp_spec) -- x_dtype the dtype of the decision's states.  A CnnSpec
        (aigar_amd.net.cnn_spec: side, channels, convs, n_flat, units, hidden, out) puts its
        conv layers in front (aigar_net_config_cnn): the states are then images [side, side,
        channels] and n_in is n_flat.  The weights are zero until net_set_weights.
        net_config(None) turns it off."""
        self.trn = self.crit = self.act = self.dpg = self.spg = None  # (the library drops the train configurations and the critic with the network)
        if spec is None:
            self._chk(self.L.aigar_net_config(self.h, None))
            self.net = self.conv = None
            return
        cprm = None
        if hasattr(spec, "convs"):
            side, channels, convs, n_flat, units, hidden, out = spec
            convs = tuple(tuple(int(v) for v in c) for c in convs)
            if not 1 <= len(convs) <= _abi.CONV_MAX_LAYERS or any(len(c) != 3 for c in convs):
                raise ValueError("net_config: 1..%d conv layers (kernel, stride, filters), got %s"
                                 % (_abi.CONV_MAX_LAYERS, convs))
            cprm = _abi.ConvParams(int(side), int(channels), len(convs))
            for i, (k, s, f) in enumerate(convs):
                cprm.k[i], cprm.stride[i], cprm.filters[i] = k, s, f
            n_in = n_flat
        else:
            n_in, units, hidden, out = spec
        prm, units, d = self._dense_params("net_config", n_in, units, hidden, out, x_dtype, 0)
        if cprm is not None:
            self._chk(self.L.aigar_net_config_cnn(self.h, C.byref(cprm), C.byref(prm)))
            self.conv = (int(side), int(channels), convs)
        else:
            self._chk(self.L.aigar_net_config(self.h, C.byref(prm)))
            self.conv = None
        self.net = (int(n_in), units, d)

    def _need_net(self, what):
        if getattr(self, "net", None) is None:
            raise RuntimeError("aigar: %s: no acting network is configured (net_config)" % what)
        return self.net

    def net_set_weights(self, weights):
        """The trainer's weight push: weights is a list of (W [in, out], b [out]) per layer,
        float32, numpy arrays or device tensors (stream-ordered; no re-capture).  With a conv
        part its layers' (W [k, k, Cin, F], b [F]) come first, then the dense pairs."""
        n_in, units, _ = self._need_net("net_set_weights")
        convs = self.conv[2] if self.conv is not None else ()
        if len(weights) != len(convs) + len(units):
            raise ValueError("net_set_weights: %d layers given, the network has %d"
                             % (len(weights), len(convs) + len(units)))
        cin = self.conv[1] if self.conv is not None else 0
        for l, (W, b) in enumerate(weights[:len(convs)]):
            k, _, f = convs[l]
            self._push_pair("net_set_weights", self.L.aigar_net_set_conv_weights, l, W, b, (k, k, cin, f))
            cin = f
        self._push_dense("net_set_weights", self.L.aigar_net_set_weights, n_in, units, weights[len(convs):])

    def net_get_weights(self, which="online", device=False):
        """The read-back of net_set_weights (aigar_net_get_weights): a list of (W [in, out],
        b [out]) float32 per dense layer, numpy arrays or (device=True) device tensors.  which:
        "online", or with a train configuration "target", "m", "v" (Adam's state)."""
        n_in, units, _ = self._need_net("net_get_weights")
        if which not in self._NET_CODES:
            raise ValueError("net_get_weights: which must be one of %s" % sorted(self._NET_CODES))
        out = []
        if self.conv is not None:  # the conv pairs first, (W [k, k, Cin, F], b [F]) (aigar_net_get_conv_weights)
            cin = self.conv[1]
            for l, (k, _, f) in enumerate(self.conv[2]):
                if device:
                    import torch
                    dev = "cuda:%d" % self.cfg.device
                    W = torch.empty((k, k, cin, f), dtype=torch.float32, device=dev)
                    b = torch.empty((f,), dtype=torch.float32, device=dev)
                else:
                    W, b = np.empty((k, k, cin, f), np.float32), np.empty((f,), np.float32)
                self._chk(self.L.aigar_net_get_conv_weights(self.h, self._NET_CODES[which], l, _ptr(W)[0], _ptr(b)[0],
                                                            int(device)))
                out.append((W, b))
                cin = f
        return out + self._read_dense("net_get_weights", self._NET_CODES, which, n_in, units, device)

    def net_pad_check(self, which="online"):
        """A debug read (aigar_net_pad_check): how many padded entries of the packed copies are
        not +0.0f (0 in every correct state; a host round trip)."""
        return self._pad_check(self._NET_CODES, which)

    # ---- the three trainers' shared plumbing: kind is the entry points' prefix
    _TRAINERS = {"train": ("trn", "no training is configured (train_config)"),
                 "actrain": ("act", "no CACLA training is configured (actrain_config)"),
                 "dpg": ("dpg", "no DPG training is configured (dpg_config)"),
                 "spg": ("spg", "no SPG training is configured (spg_config)")}

    def _need_trainer(self, kind, what):
        """The batch of the configured trainer of this kind; what: the caller, for the message."""
        attr, msg = self._TRAINERS[kind]
        if getattr(self, attr, None) is None:
            raise RuntimeError("aigar: %s: %s" % (what, msg))
        return getattr(self, attr)

    def _trainer_call(self, kind, name, *args):
        """aigar_<kind>_<name>(handle, *args) once the trainer is known to be configured."""
        self._need_trainer(kind, "%s_%s" % (kind, name))
        self._chk(getattr(self.L, "aigar_%s_%s" % (kind, name))(self.h, *args))

    def _trainer_step(self, kind, n, u):
        batch = self._need_trainer(kind, kind + "_step")
        up = self._dev_ptr(u, (int(n), batch), ("float64",), kind + "_step", optional=True)
        self._trainer_call(kind, "step", int(n), up)

    def _trainer_td(self, kind, *outs):
        """outs: (tensor or None, dtype) of every optional [batch] output, in the call's order."""
        batch = self._need_trainer(kind, kind + "_td")
        self._trainer_call(kind, "td", *[self._dev_ptr(t, (batch,), (dt,), kind + "_td", optional=True)
                                         for t, dt in outs])

    # ---- the Q-learning trainer (include/aigar.h: aigar_train*)
    def train_config(self, batch=32, min_size=0, target_steps=0, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7,
                     discount=0.85):
        """The trainer of the handle's acting network on its replay memory (aigar_train_config):
        Q-learning, Keras 2.2.4 Adam on the importance-weighted mse, a hard target copy every
        target_steps applied steps.  Needs net_config (dense, linear head), exp_config and
        decide_config.  train_config(None) turns it off."""
        if batch is None:
            self._chk(self.L.aigar_train_config(self.h, None))
            self.trn = None
            return
        prm = _abi.TrainParams(int(batch), int(min_size), int(target_steps), 0, float(lr), float(beta1), float(beta2),
                               float(epsilon), float(discount))
        self._chk(self.L.aigar_train_config(self.h, C.byref(prm)))
        self.trn = int(batch)

    def train_config_cnn(self, batch=32, min_size=0, target_steps=0, lr=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-7,
                         discount=0.85):
        """train_config for an acting network with a conv part (aigar_train_config_cnn): the same
        parameters; needs net_config with a CnnSpec (linear head) and an exp_config whose states
        are the conv part's images.  train_step, train_info, train_td, train_sync_target and
        train_reset serve it.  train_config_cnn(None) turns it off."""
        if batch is None:
            self._chk(self.L.aigar_train_config_cnn(self.h, None))
            self.trn = None
            return
        prm = _abi.TrainParams(int(batch), int(min_size), int(target_steps), 0, float(lr), float(beta1), float(beta2),
                               float(epsilon), float(discount))
        self._chk(self.L.aigar_train_config_cnn(self.h, C.byref(prm)))
        self.trn = int(batch)

    def train_step(self, n=1, u=None):
        """n training steps, one graph replay each with no host work in between
        (aigar_train_step).  u: None (the memory's own stream) or a device tensor [n, batch]
        float64 of draws in [0, 1)."""
        self._trainer_step("train", n, u)

    def train_info(self):
        """{steps, skipped, since_target} of the trainer (the one synchronising read)."""
        v = (C.c_int64 * 4)()
        self._trainer_call("train", "info", v)
        return {"steps": v[0], "skipped": v[1], "since_target": v[2]}

    def train_td(self, td=None, idx=None):
        """The last drawn step's TD errors and memory indices into the device tensors td [batch]
        float64 and idx [batch] int64 (stream-ordered copies)."""
        self._trainer_td("train", (td, "float64"), (idx, "int64"))

    def train_sync_target(self):
        self._trainer_call("train", "sync_target")

    def train_reset(self):
        self._trainer_call("train", "reset")

    # ---- the CACLA learner's critic and trainer (include/aigar.h: aigar_critic*, aigar_actrain*)
    def critic_config(self, spec, x_dtype="float64", _entry="aigar_critic_config"):
        """The handle's critic V(s): spec is (n_in, units, hidden, "linear") with units[-1] == 1 and
        the acting network's n_in (aigar_critic_config).  The weights are zero until
        critic_set_weights.  critic_config(None) turns it off."""
        config = getattr(self.L, _entry)
        self.act = self.dpg = self.spg = None  # (the library drops the train configurations with the critic)
        if spec is None:
            self._chk(config(self.h, None))
            self.crit = None
            return
        n_in, units, hidden, out = spec
        prm, units, _ = self._dense_params("critic_config", n_in, units, hidden, out, x_dtype, 1)
        self._chk(config(self.h, C.byref(prm)))
        self.crit = (int(n_in), units)

    def qcritic_config(self, spec, x_dtype="float64"):
        """The handle's critic Q(s, a) (aigar_qcritic_config): as critic_config, but n_in is the
        acting network's n_in + n_out -- a row is the state, then the action -- and the acting
        network has a sigmoid head.  critic_set_weights, critic_get_weights and critic_forward
        serve it.  qcritic_config(None) turns it off."""
        self.critic_config(spec, x_dtype, _entry="aigar_qcritic_config")

    def _need_crit(self, what):
        if getattr(self, "crit", None) is None:
            raise RuntimeError("aigar: %s: no critic is configured (critic_config)" % what)
        return self.crit

    def critic_set_weights(self, weights):
        """The critic's weights: a list of (W [in, out], b [out]) float32 per layer, numpy arrays or
        device tensors (stream-ordered)."""
        n_in, units = self._need_crit("critic_set_weights")
        if len(weights) != len(units):
            raise ValueError("critic_set_weights: %d layers given, the critic has %d" % (len(weights), len(units)))
        self._push_dense("critic_set_weights", self.L.aigar_critic_set_weights, n_in, units, weights)

    def critic_get_weights(self, which="online"):
        """[(W [in, out], b [out])] float32 numpy arrays of the critic ("online"), or with a CACLA
        train configuration of its "target", "m" or "v"."""
        n_in, units = self._need_crit("critic_get_weights")
        return self._read_dense("critic_get_weights", self._CRITIC_CODES, which, n_in, units)

    def critic_pad_check(self, which="online"):
        return self._pad_check(self._CRITIC_CODES, which)

    def critic_forward(self, x, out):
        """V(s) on device tensors (aigar_critic_forward): x [rows, n_in] float64 / float32 -> out
        [rows] float64."""
        n_in, _ = self._need_crit("critic_forward")
        rows = int(x.shape[0])
        self._forward("critic_forward", self.L.aigar_critic_forward, x, (rows, n_in), out, (rows,))

    def actrain_config(self, batch=32, min_size=0, target_steps=0, var_epochs=0, critic_lr=7.5e-5, actor_lr=5e-4,
                       beta1=0.9, beta2=0.999, epsilon=1e-7, discount=0.9, var_start=1.0, var_beta=0.001):
        """The CACLA trainer of the handle's actor and critic on its replay memory
        (aigar_actrain_config).  Needs net_config (dense, sigmoid head), critic_config and
        exp_config.  actrain_config(None) turns it off."""
        if batch is None:
            self._chk(self.L.aigar_actrain_config(self.h, None))
            self.act = None
            return
        prm = _abi.ActrainParams(int(batch), int(min_size), int(target_steps), int(var_epochs), float(critic_lr),
                                 float(actor_lr), float(beta1), float(beta2), float(epsilon), float(discount),
                                 float(var_start), float(var_beta))
        self._chk(self.L.aigar_actrain_config(self.h, C.byref(prm)))
        self.act = int(batch)

    def actrain_step(self, n=1, u=None):
        """n CACLA training steps, one graph replay each (aigar_actrain_step); u as train_step's."""
        self._trainer_step("actrain", n, u)

    def actrain_info(self):
        """The CACLA trainer's counters (aigar_actrain_info: the one synchronising read)."""
        v = (C.c_int64 * 8)()
        self._trainer_call("actrain", "info", v)
        return {"steps": v[0], "skipped": v[1], "since_target": v[2], "actor_epochs": v[3], "selected": v[4],
                "epochs": v[5], "cut": v[6], "epochs_skipped": v[7]}

    def actrain_td(self, td=None, idx=None, count=None):
        """The last drawn step's TD errors, memory indices and per-row actor epochs into the device
        tensors td [batch] float64, idx [batch] int64 and count [batch] int32."""
        self._trainer_td("actrain", (td, "float64"), (idx, "int64"), (count, "int32"))

    def actrain_var(self):
        """CACLA-Var's running variance (a host round trip)."""
        v = C.c_double()
        self._trainer_call("actrain", "var", C.byref(v))
        return float(v.value)

    def actrain_sync_target(self):
        self._trainer_call("actrain", "sync_target")

    def actrain_reset(self):
        self._trainer_call("actrain", "reset")

    # ---- the DPG trainer (include/aigar.h: aigar_dpg*)
    def dpg_config(self, batch=32, min_size=0, target_steps=0, critic_lr=5e-4, actor_lr=1e-4, beta1=0.9, beta2=0.999,
                   epsilon=1e-7, discount=0.9, tau=0.001, q_increase=2.0):
        """The DPG trainer of the handle's actor and Q(s, a) critic on its replay memory
        (aigar_dpg_config).  Needs net_config (dense, sigmoid head), qcritic_config and
        exp_config.  tau > 0: soft target updates; tau == 0: a hard copy every target_steps
        applied steps.  dpg_config(None) turns it off."""
        if batch is None:
            self._chk(self.L.aigar_dpg_config(self.h, None))
            self.dpg = None
            return
        prm = _abi.DpgParams(int(batch), int(min_size), int(target_steps), 0, float(critic_lr), float(actor_lr),
                             float(beta1), float(beta2), float(epsilon), float(discount), float(tau), float(q_increase))
        self._chk(self.L.aigar_dpg_config(self.h, C.byref(prm)))
        self.dpg = int(batch)
        self.spg = None  # (the library drops an SPG configuration for it)

    def dpg_step(self, n=1, u=None):
        """n DPG training steps, one graph replay each (aigar_dpg_step); u as train_step's."""
        self._trainer_step("dpg", n, u)

    def dpg_info(self):
        """The DPG trainer's counters (aigar_dpg_info: the one synchronising read)."""
        v = (C.c_int64 * 8)()
        self._trainer_call("dpg", "info", v)
        return {"steps": v[0], "skipped": v[1], "since_target": v[2], "actor_steps": v[3], "actor_skipped": v[4]}

    def dpg_td(self, td=None, idx=None):
        """The last drawn step's TD errors and memory indices into the device tensors td [batch]
        float64 and idx [batch] int64."""
        self._trainer_td("dpg", (td, "float64"), (idx, "int64"))

    def dpg_sync_target(self):
        self._trainer_call("dpg", "sync_target")

    def dpg_reset(self):
        self._trainer_call("dpg", "reset")

    # ---- the SPG trainer (include/aigar.h: aigar_spg*)
    def spg_config(self, batch=32, min_size=0, target_steps=0, critic_lr=5e-4, actor_lr=1e-4, beta1=0.9, beta2=0.999,
                   epsilon=1e-7, discount=0.9, tau=0.001, samples=5, moving=True, replace=True, prio_evals=True,
                   fused=True, noise=0.1, noise_decay=1.0, seed=0):
        """The SPG trainer of the handle's actor and Q(s, a) critic on its replay memory
        (aigar_spg_config): DPG's critic half, then a search of `samples` Gaussian candidates a row
        around the best action so far (moving) or the actor's, and the actor's regression towards
        the winners.  Needs what dpg_config needs and, with replace, exp_config(extra=True).  It
        and dpg_config exclude each other.  spg_config(None) turns it off."""
        if batch is None:
            self._chk(self.L.aigar_spg_config(self.h, None))
            self.spg = None
            return
        prm = _abi.SpgParams(int(batch), int(min_size), int(target_steps), 0, float(critic_lr), float(actor_lr),
                             float(beta1), float(beta2), float(epsilon), float(discount), float(tau), 0.0, int(samples),
                             int(bool(moving)), int(bool(replace)), int(bool(prio_evals)), int(bool(fused)), 0,
                             float(noise), float(noise_decay), int(seed) & (2 ** 64 - 1))
        self._chk(self.L.aigar_spg_config(self.h, C.byref(prm)))
        self.spg = (int(batch), int(samples))
        self.dpg = None  # (the library drops a DPG configuration for it)

    def spg_step(self, n=1, u=None, zu=None):
        """n SPG training steps, one graph replay each (aigar_spg_step); u as train_step's; zu:
        None (the search's own Philox draws) or a device tensor [n, batch, samples, 2, 16, 2]
        float64 of uniforms in [0, 1)."""
        batch, k = self._need_trainer("spg", "spg_step")
        up = self._dev_ptr(u, (int(n), batch), ("float64",), "spg_step", optional=True)
        zp = None if k == 0 else self._dev_ptr(zu, (int(n), batch, k, 2, 16, 2), ("float64",), "spg_step", optional=True)
        self._trainer_call("spg", "step", int(n), up, zp)

    def spg_info(self):
        """The SPG trainer's counters (aigar_spg_info: the one synchronising read)."""
        v = (C.c_int64 * 8)()
        self._trainer_call("spg", "info", v)
        return {"steps": v[0], "skipped": v[1], "since_target": v[2], "actor_steps": v[3], "actor_skipped": v[4],
                "actor_empty": v[5], "selected": v[6]}

    def spg_td(self, td=None, idx=None):
        """The last drawn step's TD errors and memory indices into the device tensors td [batch]
        float64 and idx [batch] int64."""
        batch, _ = self._need_trainer("spg", "spg_td")
        self._trainer_call("spg", "td", *[self._dev_ptr(t, (batch,), (dt,), "spg_td", optional=True)
                                          for t, dt in ((td, "float64"), (idx, "int64"))])

    def spg_noise_ptr(self):
        """The device address of the search noise's double (aigar_spg_noise)."""
        p = C.c_void_p()
        self._trainer_call("spg", "noise", C.byref(p))
        return int(p.value)

    def spg_sync_target(self):
        self._trainer_call("spg", "sync_target")

    def spg_reset(self):
        self._trainer_call("spg", "reset")

    def net_forward(self, x, out):
        """The network alone on device tensors (aigar_net_forward): x [rows, n_in] float64 /
        float32 -> out [rows, n_out] float64 (x [rows, side, side, channels] with a conv
        part).  Liveness and roles are ignored; a row whose first value is a NaN comes out NaN."""
        n_in, units, _ = self._need_net("net_forward")
        rows = int(x.shape[0])
        xshape = (rows, n_in) if self.conv is None else (rows, self.conv[0], self.conv[0], self.conv[1])
        self._forward("net_forward", self.L.aigar_net_forward, x, xshape, out, (rows, units[-1]))

    def net_output(self, out):
        """A copy of the handle's output buffer (the last decision's Q values / mu) into the
        device tensor out [NP, n_out] float64."""
        _, units, _ = self._need_net("net_output")
        self._chk(self.L.aigar_net_output(self.h, self._dev_ptr(out, (self.NP, units[-1]), ("float64",), "net_output")))

    def env_step_net(self, head, explore, reward, obs, idx=None, val=None, u=None, noisy=None, enable_split=True,
                     skip=0, params=None, n_decisions=1):
        """n_decisions whole decisions with the network in front (aigar_env_step_net), one
        graph replay each: head "q" (explore [epsilon, temperature], u [NP, 3], idx / val as
        env_step_q) or "actor" (explore [std], u [NP, 2, T, 2], noisy as env_step_ac).  obs
        must hold the current states: the network reads it, the decision rewrites it."""
        self._need_net("env_step_net")
        hd = _abi.NET_HEADS[head] if isinstance(head, str) else int(head)
        # (a dense network reads the grid row also while a pixel state is configured)
        prm, rp, op, dt = self._decision_tail("env_step_net", reward, obs, params, pixels=self.conv is not None)
        T, ip, vp, np_ = 0, None, None, None
        if hd == _abi.NET_HEAD_Q:
            ep = self._dev_ptr(explore, (2,), ("float64",), "env_step_net")
            ip = self._dev_ptr(idx, (self.NP,), ("int32",), "env_step_net")
            vp = self._dev_ptr(val, (self.NP,), ("float64",), "env_step_net")
            up = self._dev_ptr(u, (self.NP, 3), ("float64",), "env_step_net", optional=True)
        else:
            ep = self._dev_ptr(explore, (1,), ("float64",), "env_step_net")
            up, T = self._draws_arg(u, self.NP, "NP", "env_step_net")
            np_ = self._dev_ptr(noisy, (self.NP, self.net[1][-1]), ("float64",), "env_step_net", optional=True)
        self._chk(self.L.aigar_env_step_net(self.h, hd, ep, up, T, int(bool(enable_split)), int(skip), prm, rp, op, dt,
                                            ip, vp, np_, int(n_decisions)))

    # ---- action selection of the Q-learning bots (include/aigar.h: aigar_decide*)
    def decide_config(self, actions, strategy="e-Greedy", q_dtype="float32", seed=0):
        """The handle's action selection (qLearning.py:208-243): actions is the table
        [n_out, 4] (aigar_amd.actions.discrete_actions), strategy "e-Greedy" or "Boltzmann"
        (or its code), q_dtype the dtype of the Q rows, seed the salt of the own draws.
        decide_config(None) turns it off."""
        if actions is None:
            self._chk(self.L.aigar_decide_config(self.h, None, None))
            self.dec = None
            return
        t = np.ascontiguousarray(actions, np.float64)
        if t.ndim != 2 or t.shape[1] != 4:
            raise ValueError("decide_config: the action table must be [n_out, 4], got %s" % (t.shape,))
        d = _dtype_name(q_dtype, "decide_config: q_dtype")
        st = _abi.STRATEGIES[strategy] if isinstance(strategy, str) else int(strategy)
        prm = _abi.DecideParams(int(t.shape[0]), st, _dtype_code(d), 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._chk(self.L.aigar_decide_config(self.h, C.byref(prm), t.ctypes.data_as(C.c_void_p)))
        self.dec = (int(t.shape[0]), d)

    def _decide_args(self, q, explore, u, idx, val, what):
        if self.dec is None:
            raise RuntimeError("aigar: %s: no action selection is configured (decide_config)" % what)
        n, d = self.dec
        qp = self._dev_ptr(q, (self.NP, n), (d,), what)
        ep = self._dev_ptr(explore, (2,), ("float64",), what)
        ip = self._dev_ptr(idx, (self.NP,), ("int32",), what)
        vp = self._dev_ptr(val, (self.NP,), ("float64",), what)
        return qp, ep, self._dev_ptr(u, (self.NP, 3), ("float64",), what, optional=True), ip, vp

    def decide(self, q, explore, idx, val, u=None, act=None):
        """The selection alone on device tensors (aigar_decide): q [NP, n_out], explore
        [epsilon, temperature] float64, u [NP, 3] float64 draws in [0, 1) (None: the own
        Philox stream); writes idx [NP] int32, val [NP] float64 and the chosen table rows
        into act [NP, 4] (dead and non-NN players: -1, NaN, row untouched)."""
        qp, ep, up, ip, vp = self._decide_args(q, explore, u, idx, val, "decide")
        ap = self._dev_ptr(act, (self.NP, 4), ("float64",), "decide", optional=True)
        self._chk(self.L.aigar_decide(self.h, qp, ep, up, ip, vp, ap))

    def env_step_q(self, q, explore, reward, obs, idx, val, u=None, enable_split=True, skip=0, params=None):
        """One Q-learning decision on device tensors (aigar_env_step_q): decide, then
        env_step with the chosen table rows; one graph replay."""
        qp, ep, up, ip, vp = self._decide_args(q, explore, u, idx, val, "env_step_q")
        prm, rp, op, dt = self._decision_tail("env_step_q", reward, obs, params)
        self._chk(self.L.aigar_env_step_q(self.h, qp, ep, up, int(bool(enable_split)), int(skip), prm, rp, op, dt,
                                          ip, vp))

    def warnings(self, arena=0):
        """The arena's sticky quirk bits since its last reset (aigar_warnings; _abi.WARN_*)."""
        v = C.c_uint32(0)
        self._chk(self.L.aigar_warnings(self.h, int(arena), C.byref(v)))
        return v.value

    def set_actions(self, cur=None, prev=None):
        c = None if cur is None else np.ascontiguousarray(cur, np.float64)
        q = None if prev is None else np.ascontiguousarray(prev, np.float64)
        self._chk(self.L.aigar_set_actions(self.h, _ptr(c)[0], _ptr(q)[0], 0))

    def reset_bots(self, mask=None):
        """Bot.reset's device half (bot.py:125-164) for the players where mask != 0
        (all if None): history grids zeroed, lastFovSize 0."""
        p, dev = self._mask_ptr(mask)
        self._chk(self.L.aigar_reset_bots(self.h, p, dev))

    def player_stats(self):
        out = np.zeros((self.NP, 5), np.float64)
        self._chk(self.L.aigar_player_stats(self.h, out.ctypes.data_as(C.c_void_p), 0))
        return out

    def score(self, out=None):
        """[NP, 4] samples, sum, max, dead of every bot's getMassOverTime() (bot.py:253,639-640);
        needs a handle created with FLAG_SCORE.  out: numpy array or device tensor."""
        if out is None:
            out = np.zeros((self.NP, 4), np.float64)
        self._check_out(out, (self.NP, 4), ("float64",), "score")
        p, dev = _ptr(out)
        self._chk(self.L.aigar_score(self.h, p, dev))
        return out

    def score_reset(self, mask=None):
        """Bot.resetMassList for the players where mask != 0 (all if None); stream-ordered."""
        p, dev = self._mask_ptr(mask)
        self._chk(self.L.aigar_score_reset(self.h, p, dev))

    def score_trace(self, buf):
        """Attach the DEVICE tensor buf [cap, NP] float64 (row = sample index, column =
        player) as the mass lists' store, or detach with None.  The caller keeps buf alive
        while it is attached."""
        if buf is None:
            self._chk(self.L.aigar_score_trace(self.h, None, 0))
            return
        if not getattr(buf, "is_cuda", False):
            raise ValueError("score_trace: buf must be a device tensor")
        if len(buf.shape) != 2:
            raise ValueError("score_trace: buf must have shape (cap, %d), got %s" % (self.NP, tuple(buf.shape)))
        self._check_out(buf, (int(buf.shape[0]), self.NP), ("float64",), "score_trace")
        self._chk(self.L.aigar_score_trace(self.h, C.c_void_p(buf.data_ptr()), int(buf.shape[0])))

    def get_state(self, arena=0):
        cnt = _abi.State()
        self._chk(self.L.aigar_get_state(self.h, arena, C.byref(cnt)))
        st, arrays = _abi.alloc_state(cnt)
        self._chk(self.L.aigar_get_state(self.h, arena, C.byref(st)))
        return _abi.struct_to_dict(st, arrays)

    def load_state(self, d, arena=0):
        st, keep = _abi.state_to_struct(d)
        self._chk(self.L.aigar_load_state(self.h, arena, C.byref(st)))

    def events(self, arena=0):
        n = C.c_int(0)
        self._chk(self.L.aigar_get_events(self.h, arena, None, 0, C.byref(n)))
        out = np.zeros((n.value, 4), np.int64)
        if n.value:
            self._chk(self.L.aigar_get_events(self.h, arena, out.ctypes.data_as(C.POINTER(C.c_int64)), n.value,
                                              C.byref(n)))
        return out

    def events_raw(self, arena=0):
        """Unsorted event rows with their sort keys: (key_hi, key_lo, code, a, b)."""
        n = C.c_int(0)
        self._chk(self.L.aigar_get_events_raw(self.h, arena, None, 0, C.byref(n)))
        out = np.zeros((n.value, 5), np.int64)
        if n.value:
            self._chk(self.L.aigar_get_events_raw(self.h, arena, out.ctypes.data_as(C.POINTER(C.c_int64)), n.value,
                                                  C.byref(n)))
        return out

    # ---- C4 tiles (include/aigar.h: aigar_tile_*)
    def tile_info(self):
        info = (C.c_int32 * 14)()
        ob, ib, nb = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        self._chk(self.L.aigar_tile_info(self.h, info, C.byref(ob), C.byref(ib), C.byref(nb)))
        v = list(info)
        return {"ntiles": v[0], "tile_id": v[1], "own": tuple(v[2:6]), "held": tuple(v[6:10]), "tcap": v[10],
                "bm_words": v[11], "hcap": v[12], "hrec": v[13], "handoff_bytes": v[12] * v[13] * 32,
                "outbox": ob.value, "inbox": ib.value, "msg_bytes": nb.value}

    def tile_msg_bytes(self):
        """Bytes of the current pass's message (the first pass sends no bitmap)."""
        n = C.c_int64(0)
        self._chk(self.L.aigar_tile_msg_bytes(self.h, C.byref(n)))
        return n.value

    def tile_set_buffers(self, outbox_ptr, inbox_ptr):
        self._chk(self.L.aigar_tile_set_buffers(self.h, C.c_void_p(int(outbox_ptr)), C.c_void_p(int(inbox_ptr))))

    def tile_begin(self, policy="none", p_split=0.0, p_eject=0.0, seed=0):
        """policy "greedy": this tick's commands must have gone round already
        (tile_policy, the exchange, tile_apply_commands)."""
        pol = {"none": _abi.POLICY_NONE, "random": _abi.POLICY_RANDOM, "greedy": _abi.POLICY_GREEDY}[policy]
        prm = _abi.RunParams(pol, 0, float(p_split), float(p_eject), int(seed))
        self._chk(self.L.aigar_tile_begin(self.h, C.byref(prm)))

    def tile_policy(self, greedy_split=False):
        """Greedy moves (bot.py:579-633) of the bots this tile observes, into the
        command message the transport all-gathers next."""
        self._chk(self.L.aigar_tile_policy(self.h, 1 if greedy_split else 0))

    def tile_apply_commands(self):
        """The other tiles' Greedy commands (after the exchange of tile_policy's messages)."""
        self._chk(self.L.aigar_tile_apply_commands(self.h))

    def tile_apply(self, wait=True):
        """Apply the gathered messages; wait: return the owned cells still undone on
        all tiles (a host round trip), else None (the next pass gates itself)."""
        if not wait:
            self._chk(self.L.aigar_tile_apply(self.h, None))
            return None
        u = C.c_int(0)
        self._chk(self.L.aigar_tile_apply(self.h, C.byref(u)))
        return u.value

    def tile_observers(self):
        """Per player: the tile that computed its row at the last observation (-1: dead)."""
        out = np.zeros(self.NP, np.int32)
        self._chk(self.L.aigar_tile_observers(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def tile_resume(self):
        self._chk(self.L.aigar_tile_resume(self.h))

    def tile_comm_init(self, uid, nranks, rank):
        """This tile's RCCL communicator (ncclCommInitRank): nranks = tiles, rank = tile id."""
        path = rccl_path()
        buf = C.create_string_buffer(bytes(uid), 128)
        self._chk(self.L.aigar_tile_comm_init(self.h, path.encode() if path else None, buf, int(nranks), int(rank)))

    def tile_run(self, n=1, policy="random", out=None, p_split=0.0, p_eject=0.0, seed=0, extra_passes=0,
                 greedy_split=False):
        """n tiled steps over RCCL (aigar_tile_run): policy (greedy: each tile moves the bots
        it observes, the commands all-gathered first) + the tick with its all-gathered eat
        passes + the observation of this tile's bots into the DEVICE tensor out."""
        pol = {"none": _abi.POLICY_NONE, "random": _abi.POLICY_RANDOM, "greedy": _abi.POLICY_GREEDY}[policy]
        prm = _abi.RunParams(pol, 1 if greedy_split else 0, float(p_split), float(p_eject), int(seed))
        p, dt = None, 0
        if out is not None:
            if not getattr(out, "is_cuda", False) or tuple(out.shape) != (self.NP, self.obs_len):
                raise ValueError("tile_run writes observations to a device tensor [%d, %d]" % (self.NP, self.obs_len))
            dt = _dtype_code(_dtype_name(out.dtype))
            p = C.c_void_p(out.data_ptr())
        self._chk(self.L.aigar_tile_run(self.h, int(n), C.byref(prm), int(extra_passes), p, dt))

    def tile_run_graphed(self):
        return bool(self.L.aigar_tile_run_graphed(self.h))

    def tile_loopback(self):
        """Timing rehearsal (include/aigar.h aigar_tile_loopback): tile_run without a
        communicator, every other tile's message empty."""
        self._chk(self.L.aigar_tile_loopback(self.h))

    def tile_end(self, out=None):
        p, dt = None, 0
        if out is not None:
            if not getattr(out, "is_cuda", False) or tuple(out.shape) != (self.NP, self.obs_len):
                raise ValueError("tile_end writes observations to a device tensor [%d, %d]" % (self.NP, self.obs_len))
            dt = _dtype_code(_dtype_name(out.dtype))
            p = C.c_void_p(out.data_ptr())
        self._chk(self.L.aigar_tile_end(self.h, p, dt))

    COUNTERS = ("vb_serial", "pv_serial", "food_serial", "pellets_eaten", "pp_serial_players", "pellets_spawned",
                "pp_parallel_ticks",
                "ticks")

    def counters(self, arena=0):
        out = np.zeros(8, np.int64)
        self._chk(self.L.aigar_counters(self.h, arena, out.ctypes.data_as(C.POINTER(C.c_int64)), 8))
        return {k: int(v) for k, v in zip(self.COUNTERS, out) if k != "-"}

    def set_stream(self, stream_ptr):
        self._chk(self.L.aigar_set_stream(self.h, C.c_void_p(int(stream_ptr))))

    def sync(self):
        self._chk(self.L.aigar_sync(self.h))

    def profile(self, enable=True):
        self._chk(self.L.aigar_profile(self.h, int(bool(enable))))

    def kernel_time(self, name):
        ms, n = C.c_double(0), C.c_int(0)
        self._chk(self.L.aigar_kernel_time(self.h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


def tile_exchange_local(steppers):
    """In-process transport of a tiled arena: every tile's outbox into every tile's inbox."""
    L = load()
    arr = (C.c_void_p * len(steppers))(*[s.h.value for s in steppers])
    if L.aigar_tile_exchange_local(arr, len(steppers)) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())


def selftest_trig(y, x):
    """Device atan2(y, x), sin(x), cos(x) (glibc's, restated in aigar_glibc_trig.h) for host arrays."""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    out = np.zeros(3 * len(x))
    dp = C.POINTER(C.c_double)
    if L.aigar_selftest_trig(y.ctypes.data_as(dp), x.ctypes.data_as(dp), out.ctypes.data_as(dp), len(x)) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())
    n = len(x)
    return out[:n], out[n:2 * n], out[2 * n:]


def selftest_pow(x, y):
    """Device pow (glibc's, restated in aigar_math.h) for host arrays (diagnostics)."""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    y = np.ascontiguousarray(y, np.float64)
    out = np.zeros_like(x)
    dp = C.POINTER(C.c_double)
    if L.aigar_selftest_pow(x.ctypes.data_as(dp), y.ctypes.data_as(dp), out.ctypes.data_as(dp), len(x)) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())
    return out


def selftest_log(x):
    """Device log (glibc's, restated in aigar_math.h) for a host array (diagnostics)."""
    L = load()
    x = np.ascontiguousarray(x, np.float64)
    out = np.zeros_like(x)
    dp = C.POINTER(C.c_double)
    if L.aigar_selftest_log(x.ctypes.data_as(dp), out.ctypes.data_as(dp), len(x)) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())
    return out


def selftest_sem(op, *columns):
    """Device helpers of aigar_sem.h / aigar_math.h (include/aigar.h: aigar_selftest_sem) on host
    columns of equal length: op is an _abi.SEM_* code, the result a tuple of the op's output
    columns.  float64 columns are values; uint64 columns (the Philox op's words) go and come
    back as bit patterns, viewed as float64: view an output as uint64 to read its word."""
    L = load()
    if op not in _abi.SEM_COLS:
        raise ValueError("selftest_sem: op %r is no _abi.SEM_* code" % (op,))
    n_in, n_out = _abi.SEM_COLS[op]
    if len(columns) != n_in:
        raise ValueError("selftest_sem: op %d takes %d columns, got %d" % (op, n_in, len(columns)))
    cols = []
    for c in columns:
        c = np.asarray(c)
        cols.append(c.view(np.float64) if c.dtype == np.uint64 else c.astype(np.float64, copy=False))
    n = len(cols[0])
    if any(c.shape != (n,) for c in cols):
        raise ValueError("selftest_sem: columns of unequal length")
    src = np.ascontiguousarray(np.stack(cols)) if n else np.zeros((n_in, 0))
    out = np.zeros((n_out, n))
    dp = C.POINTER(C.c_double)
    if L.aigar_selftest_sem(op, src.ctypes.data_as(dp), n_in, out.ctypes.data_as(dp), n_out, n) < 0:
        raise RuntimeError("aigar: " + L.aigar_last_error().decode())
    return tuple(out)
