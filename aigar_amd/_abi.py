"""ctypes mirror of include/aigar.h (the C-ABI of libaigar_hip.so).

Only plain structs and numpy conversion helpers live here; loading the HIP
library is in `_lib.py`.
"""
import ctypes as C

import numpy as np

ABI_VERSION = 7

RNG_PHILOX = 0
RNG_MT19937 = 1

OBS_PELLET, OBS_SELF, OBS_WALL, OBS_ENEMY, OBS_ALL, OBS_VIRUS = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
OBS_SELF_SLF, OBS_SELF_LF, OBS_ENEMY_SLF, OBS_ENEMY_LF = 0x40, 0x80, 0x100, 0x200
OBS_SIMPLE = 0x400  # GRID_VIEW_ENABLED = False: getSimpleStateRepresentation, 12 values
EX_LAST_FOV, EX_FOV, EX_MASS, EX_LAST_ACT, EX_2LAST_ACT = 0x1, 0x2, 0x4, 0x8, 0x10

EV_MERGE, EV_VIRUS_EAT_BLOB, EV_VIRUS_SPLIT, EV_CELL_EAT_VIRUS, EV_EXPLODE = 1, 2, 3, 4, 5
EV_CELL_EAT_PELLET, EV_CELL_EAT_BLOB, EV_CELL_EAT_CELL, EV_PLAYER_DEATH, EV_RESPAWN = 6, 7, 8, 9, 10

FLAG_EVENTS = 0x1
FLAG_SCORE = 0x2  # per-player mass history statistics (Stepper.score*, AgarVecEnv(score=True))
TILE_OWNED_ONLY = 0x1
TILE_FORCE = 0x2  # a 1 x 1 tiled handle (the whole field one tile: the one-GPU test of the exchange path)


PIX_RGB, PIX_LAST = 0x1, 0x2  # aigar_pixel_params.flags
POLICY_NONE, POLICY_RANDOM, POLICY_GREEDY = 0, 1, 2
ROLE_NN, ROLE_GREEDY, ROLE_RANDOM = 0, 1, 2
ROLES = {"NN": ROLE_NN, "Greedy": ROLE_GREEDY, "Random": ROLE_RANDOM}


class EnvParams(C.Structure):
    """aigar_env_params (include/aigar.h): the device Greedy / Random bots of a mixed population."""
    _fields_ = [("greedy_split", C.c_int32), ("random_skip", C.c_int32), ("random_split", C.c_int32),
                ("random_eject", C.c_int32), ("salt", C.c_uint64)]


class PixelParams(C.Structure):
    """aigar_pixel_params (include/aigar.h): the learner's pixel state (CNN_P_REPR)."""
    _fields_ = [("side", C.c_int32), ("flags", C.c_int32), ("color_seed", C.c_uint64)]


EXP_PRIORITIZED = 0x1  # aigar_exp_params.flags
EXP_EXTRA = 0x2  # ... the tuple's fifth field (CACLA's raw action, SPG's best action)


class ExpParams(C.Structure):
    """aigar_exp_params (include/aigar.h): the learners' replay memory (replay_buffer.py)."""
    _fields_ = [("capacity", C.c_int64), ("state_dtype", C.c_int32), ("flags", C.c_int32), ("alpha", C.c_double),
                ("beta", C.c_double), ("seed", C.c_uint64)]


DECIDE_EGREEDY, DECIDE_BOLTZMANN = 0, 1  # aigar_decide_params.strategy (EXPLORATION_STRATEGY)
STRATEGIES = {"e-Greedy": DECIDE_EGREEDY, "Boltzmann": DECIDE_BOLTZMANN}
DECIDE_MAX_OUT = 1024
WARN_Q_NONFINITE = 0x8  # aigar_warnings: a live player's Q row held a NaN or an infinity


class DecideParams(C.Structure):
    """aigar_decide_params (include/aigar.h): the Q-learning bots' action selection (qLearning.py:208-243)."""
    _fields_ = [("n_out", C.c_int32), ("strategy", C.c_int32), ("q_dtype", C.c_int32), ("pad", C.c_int32),
                ("seed", C.c_uint64)]


NOISE_GAUSSIAN, NOISE_ORN_UHL = 0, 1  # aigar_noise_params.type (NOISE_TYPE)
NOISE_TYPES = {"Gaussian": NOISE_GAUSSIAN, "Orn-Uhl": NOISE_ORN_UHL}
NOISE_MAX_T = 16
WARN_NOISE_NONFINITE = 0x10  # aigar_warnings: a deciding row's mu or the std was not finite (taken as 0)
WARN_NOISE_EXHAUSTED = 0x20  # aigar_warnings: a pair's attempts were all rejected (the pair is (0.0, 0.0))


class NoiseParams(C.Structure):
    """aigar_noise_params (include/aigar.h): the actor-critic learners' exploration noise (actorCritic.py:922-936)."""
    _fields_ = [("n_act", C.c_int32), ("type", C.c_int32), ("mu_dtype", C.c_int32), ("store_raw", C.c_int32),
                ("theta", C.c_double), ("ou_mu", C.c_double), ("dt", C.c_double), ("seed", C.c_uint64)]


# aigar_selftest_sem's ops (include/aigar.h AIGAR_SEM_*) and their (input, output) column counts
(SEM_MOD_POS, SEM_TRUNC_DIV_POS, SEM_PY_MOD, SEM_ROUND3, SEM_SUM, SEM_RADIUS, SEM_BUCKET, SEM_FOOTPRINT, SEM_MOVE,
 SEM_MOMENTUM, SEM_MERGE_TIME, SEM_PHILOX, SEM_TRIG_FORMS) = range(13)
SEM_COLS = {SEM_MOD_POS: (2, 1), SEM_TRUNC_DIV_POS: (2, 1), SEM_PY_MOD: (2, 1), SEM_ROUND3: (1, 1), SEM_SUM: (17, 2),
            SEM_RADIUS: (1, 2), SEM_BUCKET: (2, 3), SEM_FOOTPRINT: (4, 4), SEM_MOVE: (6, 4), SEM_MOMENTUM: (7, 2),
            SEM_MERGE_TIME: (2, 1), SEM_PHILOX: (8, 6), SEM_TRIG_FORMS: (2, 6)}


NET_MAX_LAYERS, NET_MAX_UNITS, NET_MAX_IN = 5, 256, 16384  # aigar_net_params' bounds
ACT_LINEAR, ACT_RELU, ACT_SIGMOID, ACT_ELU, ACT_TANH = 0, 1, 2, 3, 4  # (elu and tanh are refused)
ACTIVATIONS = {"linear": ACT_LINEAR, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID, "elu": ACT_ELU, "tanh": ACT_TANH}
NET_HEAD_Q, NET_HEAD_ACTOR = 0, 1  # aigar_env_step_net's head
NET_HEADS = {"q": NET_HEAD_Q, "actor": NET_HEAD_ACTOR}


class NetParams(C.Structure):
    """aigar_net_params (include/aigar.h): the learners' acting network (network.py:207-241)."""
    _fields_ = [("n_layers", C.c_int32), ("n_in", C.c_int32), ("x_dtype", C.c_int32), ("hidden_act", C.c_int32),
                ("out_act", C.c_int32), ("pad", C.c_int32), ("units", C.c_int32 * 8)]


TRAIN_MAX_BATCH = 256
WARN_TRAIN_NONFINITE = 0x40  # aigar_warnings (arena 0): a training step met a non-finite TD error and was skipped
NET_ONLINE, NET_TARGET, NET_ADAM_M, NET_ADAM_V = 0, 1, 2, 3  # aigar_net_get_weights' which


class TrainParams(C.Structure):
    """aigar_train_params (include/aigar.h): the Q-learning trainer (qLearning.py:116-193; Keras 2.2.4 Adam)."""
    _fields_ = [("batch", C.c_int32), ("min_size", C.c_int32), ("target_steps", C.c_int32), ("pad", C.c_int32),
                ("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("epsilon", C.c_double),
                ("discount", C.c_double)]


ACTRAIN_MAX_EPOCHS = 8
# aigar_net_get_weights' which, the CACLA learner's: the critic, its target, its Adam m and v
NET_CRITIC, NET_CRITIC_TARGET, NET_CRITIC_M, NET_CRITIC_V = 4, 5, 6, 7


class ActrainParams(C.Structure):
    """aigar_actrain_params (include/aigar.h): the CACLA trainer (actorCritic.py:791-858, 1032-1065)."""
    _fields_ = [("batch", C.c_int32), ("min_size", C.c_int32), ("target_steps", C.c_int32), ("var_epochs", C.c_int32),
                ("critic_lr", C.c_double), ("actor_lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("epsilon", C.c_double), ("discount", C.c_double), ("var_start", C.c_double), ("var_beta", C.c_double)]


class DpgParams(C.Structure):
    """aigar_dpg_params (include/aigar.h): the DPG trainer (actorCritic.py:751-789, 986-1029)."""
    _fields_ = [("batch", C.c_int32), ("min_size", C.c_int32), ("target_steps", C.c_int32), ("reserved", C.c_int32),
                ("critic_lr", C.c_double), ("actor_lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
                ("epsilon", C.c_double), ("discount", C.c_double), ("tau", C.c_double), ("q_increase", C.c_double)]


SPG_MAX_SAMPLES = 8


class SpgParams(C.Structure):
    """aigar_spg_params (include/aigar.h): the SPG trainer (actorCritic.py:860-919, 986-1029)."""
    _fields_ = DpgParams._fields_ + [("samples", C.c_int32), ("moving", C.c_int32), ("replace", C.c_int32),
                                     ("prio_evals", C.c_int32), ("fused", C.c_int32), ("pad", C.c_int32),
                                     ("noise", C.c_double), ("noise_decay", C.c_double), ("seed", C.c_uint64)]


CONV_MAX_LAYERS, CONV_MAX_SIDE, CONV_MAX_CHANNELS, CONV_MAX_KERNEL, CONV_MAX_FILTERS = 3, 128, 8, 8, 64


class ConvParams(C.Structure):
    """aigar_conv_params (include/aigar.h): the conv part of the CNN learners' acting network
    (network.py:154-183)."""
    _fields_ = [("side", C.c_int32), ("channels", C.c_int32), ("n_conv", C.c_int32), ("k", C.c_int32 * 3),
                ("stride", C.c_int32 * 3), ("filters", C.c_int32 * 3)]


class RunParams(C.Structure):
    """aigar_run_params (include/aigar.h): the policy replayed inside aigar_run's step graph."""
    _fields_ = [("policy", C.c_int32), ("greedy_split", C.c_int32), ("p_split", C.c_double),
                ("p_eject", C.c_double), ("seed", C.c_uint64)]


class RewardParams(C.Structure):
    """aigar_reward_params (include/aigar.h); defaults of networkParameters.py:50,69-72."""
    _fields_ = [("mass_as_reward", C.c_int32), ("pad", C.c_int32), ("reward_term", C.c_double),
                ("death_term", C.c_double), ("death_factor", C.c_double), ("reward_scale", C.c_double)]

    @classmethod
    def from_parameters(cls, p=None):
        g = (lambda n, dflt: getattr(p, n, dflt)) if p is not None else (lambda n, dflt: dflt)
        return cls(int(bool(g("MASS_AS_REWARD", False))), 0, float(g("REWARD_TERM", 0)), float(g("DEATH_TERM", -40)),
                   float(g("DEATH_FACTOR", 1.5)), float(g("REWARD_SCALE", 2)))


class Config(C.Structure):
    _fields_ = [
        ("n_arenas", C.c_int32), ("bots_per_arena", C.c_int32), ("field_size", C.c_int32),
        ("virus_enabled", C.c_int32), ("max_pellets", C.c_double), ("max_viruses", C.c_double),
        ("grid_squares", C.c_int32), ("obs_channels", C.c_uint32), ("obs_extras", C.c_uint32),
        ("rng_mode", C.c_int32), ("device", C.c_int32), ("pellet_cap", C.c_int32),
        ("blob_cap", C.c_int32), ("virus_cap", C.c_int32), ("event_cap", C.c_int32), ("flags", C.c_int32),
        ("tile_x", C.c_int32), ("tile_y", C.c_int32), ("tile_id", C.c_int32), ("tile_halo", C.c_int32),
        ("tile_cap", C.c_int32), ("tile_flags", C.c_int32),
    ]


_PD = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int64)


class State(C.Structure):
    _fields_ = [
        ("n_players", C.c_int32), ("field_size", C.c_int32), ("virus_enabled", C.c_int32), ("rng_mode", C.c_int32),
        ("seq_next", C.c_int64), ("tick", C.c_int64),
        ("max_pellets", C.c_double), ("max_viruses", C.c_double),
        ("philox_key", C.c_uint64 * 2), ("ctr_pellet", C.c_uint64), ("ctr_virus", C.c_uint64),
        ("mt_key", C.c_uint32 * 624), ("mt_pos", C.c_int32),
        ("n_cells", C.c_int32), ("n_pellets", C.c_int32), ("n_blobs", C.c_int32), ("n_viruses", C.c_int32),
        ("n_dead", C.c_int32),
        ("players_f", _PD), ("players_i", _PI), ("cells_f", _PD), ("cells_i", _PI),
        ("pellets_f", _PD), ("pellets_seq", _PI), ("blobs_f", _PD), ("blobs_i", _PI),
        ("viruses_f", _PD), ("viruses_i", _PI), ("dead", _PI),
        ("pellets_col", _PI), ("blobs_col", _PI),
    ]


# snapshot record layouts: name -> (count field, columns, dtype)
LAYOUT = {
    "players_f": ("n_players", 2, np.float64), "players_i": ("n_players", 5, np.int64),
    "cells_f": ("n_cells", 9, np.float64), "cells_i": ("n_cells", 4, np.int64),
    "pellets_f": ("n_pellets", 4, np.float64), "pellets_seq": ("n_pellets", 0, np.int64),
    "blobs_f": ("n_blobs", 8, np.float64), "blobs_i": ("n_blobs", 3, np.int64),
    "viruses_f": ("n_viruses", 8, np.float64), "viruses_i": ("n_viruses", 3, np.int64),
    "dead": ("n_dead", 0, np.int64),
    # optional: colour owners (player index, -1: own colour); absent from older snapshots
    "pellets_col": ("n_pellets", 0, np.int64), "blobs_col": ("n_blobs", 0, np.int64),
}
OPTIONAL = ("pellets_col", "blobs_col")
SCALARS = ("n_players", "field_size", "virus_enabled", "rng_mode", "seq_next", "tick",
           "max_pellets", "max_viruses", "ctr_pellet", "ctr_virus", "mt_pos")


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def state_to_struct(d):
    """numpy snapshot dict -> (State, keepalive list)."""
    st = State()
    keep = []
    for name, (cnt, cols, dt) in LAYOUT.items():
        if name in OPTIONAL and name not in d:
            continue  # (NULL: the library takes -1)
        a = np.ascontiguousarray(d[name], dtype=dt)
        n = a.shape[0] if a.ndim else 0
        if cols:
            a = a.reshape(n, cols)
        keep.append(a)
        if cnt != "n_players":
            setattr(st, cnt, n)
        setattr(st, name, _ptr(a, C.c_double if dt == np.float64 else C.c_int64))
    for k in SCALARS:
        if k in d:
            setattr(st, k, float(d[k]) if k.startswith("max_") else int(d[k]))
    st.n_players = int(d["players_f"].shape[0])
    if "philox_key" in d:
        st.philox_key[0], st.philox_key[1] = int(d["philox_key"][0]), int(d["philox_key"][1])
    if "mt_key" in d:
        C.memmove(st.mt_key, np.ascontiguousarray(d["mt_key"], np.uint32).ctypes.data, 624 * 4)
    return st, keep


def alloc_state(counts):
    """Allocate arrays for a State whose counts were filled by a NULL-array query."""
    st = State()
    C.memmove(C.byref(st), C.byref(counts), C.sizeof(State))
    arrays = {}
    for name, (cnt, cols, dt) in LAYOUT.items():
        n = getattr(st, cnt)
        a = np.zeros((n, cols) if cols else (n,), dtype=dt)
        arrays[name] = a
        setattr(st, name, _ptr(a, C.c_double if dt == np.float64 else C.c_int64))
    return st, arrays


def struct_to_dict(st, arrays):
    d = dict(arrays)
    for k in SCALARS + ("n_cells", "n_pellets", "n_blobs", "n_viruses", "n_dead"):
        d[k] = getattr(st, k)
    d["philox_key"] = np.array([st.philox_key[0], st.philox_key[1]], np.uint64)
    d["mt_key"] = np.frombuffer(bytes(st.mt_key), dtype=np.uint32).copy()
    return d


def obs_len(grid_squares, channels, extras):
    if channels & OBS_SIMPLE:
        return 12
    g = grid_squares or 11
    n = bin(channels & 0x3FF).count("1")
    e = (1 if extras & EX_LAST_FOV else 0) + (1 if extras & EX_FOV else 0) + (1 if extras & EX_MASS else 0) \
        + (4 if extras & EX_LAST_ACT else 0) + (4 if extras & EX_2LAST_ACT else 0)
    return g * g * n + e
