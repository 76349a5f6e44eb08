"""Vectorised environment for learners (NN-bot glue).

Replaces the reference's per-bot NN plumbing -- Bot.move_NN / updateRewards /
updateFrameSkip / updateValues (bot.py:166-233) driven by
`aigar.py:performModelSteps` (aigar.py:795-887) -- with batched device calls:
the NN players' actions come from the learner as one [n_players, n_act]
tensor.  All tensors stay on the GPU (torch-ROCm).

Populations (aigar.py:767-780 trains NN bots among Greedy and Random bots):
`roles` gives every player of an arena "NN", "Greedy" or "Random".  The Greedy
bots (bot.py:579-633) and the Random bots (bot.py:243-249: a new random action
every FRAME_SKIP_RATE moves) move on the device every tick; the learner's
actions apply to the NN players only, and only they are observed.

Per decision (`step`): the NN actions go through set_command_point and are held
for FRAME_SKIP_RATE + 1 ticks with split/eject dropped on the skipped ticks;
the reward is the reference's cumulative reward over the window (getReward
each tick against the lastMass the player had when it decided, bot.py:228-230;
nothing for a player without one, bot.py:167); the observation is
Bot.getStateRepresentation of every NN player (NaN rows for dead players, where
the reference returns None).

Pixel states: with CNN_REPR and CNN_P_REPR (or `pixels=(side, rgb, last)`) the
state is the reference's pixel frame through (frame - 255) / 100 (bot.py:276-282),
`obs` is [NP, side, side, C] of `pixel_dtype`, and everything above holds for it:
masked to the NN players, NaN rows for dead players, the previous frame (`last`)
reset with the bot, the same one graph replay per decision.

Episodes (aigar.py:833-837, 876-887): an arena's episode ends after the
decision in which its tick count passes RESET_LIMIT - FRAME_SKIP_RATE + 2 (the
reference's collector test); the arena is then reset (Model.resetModel + the
bots' reset) and reported in `done`.  With several arenas the game stages are
desynchronised the way the reference desynchronises its collectors: before the
first decision arena k has played k * int(RESET_LIMIT / n_arenas) ticks of its
own world with its own population (the NN players on random actions during
that warm-up, the reference's untrained networks), then every bot is reset
(Model.resetBots).

Scores (`score=True`; aigar.py:523-538 performAgarioTest): every tick starts with
each bot's mass sample on the device (Bot.makeMove, bot.py:253).  `score()` gives
the running episodes' [NP, 4] samples / sum / max / deaths; when an arena's episode
ends its rows move to `last_score` (and the NN players' summed rewards to
`last_return`) before the arena is reset, and `test_score()` reduces them to the
reference's meanMass and maxMass per arena.  The warm-up is not scored.

Replay memory (`memory=True` or a dict; replay_buffer.py, aigar.py:1109-1125): the
stepper keeps the learners' experience replay memory on the device.  Every `step`
appends, inside its graph, the NN players' (oldState, action, reward, newState, done)
transitions of bot.py:204-217 (a dead player's newState is a NaN row and done is set;
a time-limit end is not a done, aigar.py:851-887); `sample()` draws a mini-batch into
device tensors, uniform or prioritized with importance weights, and
`update_priorities()` writes the trainer's |td| + 1e-4 back (aigar.py:1075-1086).
`memory=True` reads MEMORY_CAPACITY, PRIORITIZED_EXP_REPLAY_ENABLED, MEMORY_ALPHA,
MEMORY_BETA and MEMORY_BATCH_LEN from `parameters`; a dict (capacity, prioritized,
alpha, beta, batch, seed) overrides them.  It is never switched on by `parameters` alone.

Q-learning (`discrete=True` or a dict; qLearning.py:208-243, network.py:26-65): the learner's
network gives one value per discrete action, and `step_q(q)` makes the reference's decideMove
for every live NN player on the device, inside the decision's graph: the e-Greedy coin, the
Boltzmann draw or argmax, then the row of the action table as the 4-value action.  `actions` is
the table, `explore` the device tensor [epsilon, temperature] the decision reads (write it, or
call `set_exploration`, to follow a decay schedule: no re-capture), `action_idx` and
`action_value` the chosen indices and the reference's qValues entries (NaN when exploring, the
probability under Boltzmann).  With a replay memory the stored action row is [index, 0, 0, 0]
(bot.py:206).  `discrete=True` reads NUM_ACTIONS, SQUARE_ACTIONS, EXPLORATION_STRATEGY, EPSILON
and TEMPERATURE from `parameters`; a dict (num_actions, square, strategy, seed) overrides them.
All players of one decision see the same epsilon and temperature; the decay schedule stays
with the caller.  It is never switched on by `parameters` alone.

Actor-critic learners (`continuous=True` or a dict; actorCritic.py:922-966, CACLA / DPG / SPG):
the learner's actor gives n_act = 2 + ENABLE_SPLIT + ENABLE_EJECT numbers in [0, 1] per player,
and `step_ac(mu)` makes the reference's applyNoise for every live NN player on the device, inside
the decision's graph: numpy's legacy Gaussian or the Ornstein-Uhlenbeck recurrence (one state per
player, cleared with the bot's history), the clip to [0, 1], then the move by the noisy action,
which stays in `noisy_action` (NaN rows where nobody decided).  `noise_std` is the device tensor
[std] the decision reads (write it, or call `set_noise`, to follow AC_NOISE_DECAY: no re-capture).
`perturb(actions)` is the noise alone on any rows (SPG's offline exploration).  With a replay
memory the stored action is the noisy one and the tuple's fifth field (bot.py:206-216) is kept:
the raw action when ALGORITHM is "CACLA", else empty until `update_actions(idx, actions)` writes
the best sampled action back (replay_buffer.py update_dones); `sample_extra(idx)` reads it.
`continuous=True` reads NOISE_TYPE, ORN_UHL_THETA / MU / DT, GAUSSIAN_NOISE and ALGORITHM from
`parameters`; a dict (noise, theta, mu, dt, std, store_raw, seed) overrides them.  It excludes
`discrete=` and is never switched on by `parameters` alone.

The acting network (`network=True` or a spec, with `discrete=` or `continuous=`):
the learner's acting MLP runs on the device in front of the selection or the noise, inside the
decision's graph, so a decision needs nothing from the host: `step_net()` is `step_q(q_network(obs))`
or `step_ac(actor(obs))` with the network evaluated by the device from `obs`, the buffer the last
decision (or `reset` / `observe`) left the states in; `collect(n)` is n such decisions back to back,
split only where an episode ends; `set_weights(weights)` is the trainer's push (no re-capture) and
`net_output` a clone of the last decision's Q values or mu.  `network=True` builds the spec from
`parameters` (aigar_amd.net.mlp_spec: Q_LAYERS / CACLA_ACTOR_LAYERS / DPG_ACTOR_LAYERS and the
activations; what the device cannot evaluate is refused there); a (n_in, units, hidden, out) tuple
overrides it.  The weights are zero until the first `set_weights`.  Epsilon, temperature and the
noise level are read from `explore` / `noise_std` at every decision, so `collect(n)` uses what
they hold for all n: a decay schedule is written between calls.
The CACLA trainer (`train=True` or a dict, with `continuous=`, `network=` and `memory=`):
the reference's default learner (actorCritic.py, ALGORITHM "CACLA", CACLA-Var included) on the device.
The critic V(s) is a second network of the handle (`critic=` overrides aigar_amd.net.critic_spec's
CACLA_CRITIC_LAYERS); `train(n)` makes n steps -- the critic's update, then the actor's epochs on the
rows with a positive TD error, in place on the acting network's weights -- one graph replay each, and
the next `collect` acts with the trained actor.  `set_critic_weights()`, `get_critic_weights(target=)`,
`critic_value(states)` and `cacla_var()` reach the critic and the variance; `train_info()` has this
learner's counters.  `train=True` reads CACLA_CRITIC_ALPHA, CACLA_ACTOR_ALPHA, DISCOUNT,
TARGET_NETWORK_STEPS, NUM_EXPS_BEFORE_TRAIN, CACLA_VAR_ENABLED / _START / _BETA; what the device does
not do is refused by name (aigar_amd.net.actrain_params).
The DPG trainer (`train="dpg"` or `train=dict(algorithm="dpg", ...)`, with `continuous=`, `network=` and
`memory=`): the reference's third learner (actorCritic.py, ALGORITHM "DPG") on the device.
The critic Q(s, a) takes the action beside the state (`critic=` overrides aigar_amd.net.qcritic_spec's
DPG_CRITIC_LAYERS / DPG_CRITIC_FUNC; its n_in is the actor's n_in + n_out); the actor and the critic
each have a target, updated softly (SOFT_TARGET_UPDATES, DPG_TAU) or by a hard copy every
TARGET_NETWORK_STEPS.  `train(n)` makes n steps -- the critic's TD update, then the actor's step along
dQ/da through the updated critic, then the target update -- one graph replay each.  `get_weights(target=True)`
is the actor's target, `get_critic_weights(target=)` the critic's, `q_value(states, actions)` evaluates
the critic; `train_info()` has steps, skipped, since_target, actor_steps and actor_skipped.  What the
device does not do is refused by name (aigar_amd.net.dpg_params).
The Q-learning trainer (`train=True` or a dict, with `discrete=`, `network=` and `memory=`):
the reference's Q-learning trainer (qLearning.py:116-193, Keras 2.2.4 Adam on the importance-weighted
mse, a hard target copy every TARGET_NETWORK_STEPS) on the device, in place on the acting network's
weights: `train(n)` makes n steps on the replay memory, one graph replay each, and the next decision
acts with the trained weights; `get_weights()` reads them back, `train_info()` the counters.
`train=True` reads ALPHA, DISCOUNT, TARGET_NETWORK_STEPS, NUM_EXPS_BEFORE_TRAIN and the memory's batch;
a dict (batch, min_size, target_steps, lr, beta1, beta2, epsilon, discount) overrides them.  Every
other optimiser setting of the reference is refused by name (aigar_amd.net.train_params).  It is never
switched on by `parameters` alone.

With a pixel state (`pixels=` or CNN_REPR and CNN_P_REPR) the network is the reference's CNN
(DESIGN.md §4k): `network=True` builds a CnnSpec from `parameters` (aigar_amd.net.cnn_spec: CNN_L1/2/3,
CNN_USE_L1/2/3 and the dense settings above), a CnnSpec overrides it; the conv layers run on the
device too, in the same graph, and `set_weights` takes the conv pairs first (a torch module of
nn.Conv2d and nn.Linear layers is converted, aigar_amd.net.cnn_weights_from_torch).  With
`discrete=`, `memory=` and `train=` the CNN is trained on the device as the MLP is (DESIGN.md §4p:
the conv layers' backward pass and Adam on the packed filters, in the step's graph); `get_weights()`
then returns the conv pairs first (aigar_amd.net.cnn_weights_to_torch).  With `continuous=` a pixel
state is not trained on the device.
"""
import collections

import numpy as np

from . import _abi, actions as _actions, net as _net
from ._lib import Stepper
from .model import obs_masks, pixel_params


Batch = collections.namedtuple("Batch", "s a r s2 done w idx")


def _settings(name, defaults, given):
    """The settings of an option that is True or a dict: the defaults (read from `parameters`),
    overridden by the dict's entries; a key that is no setting is refused under the option's name."""
    if isinstance(given, dict):
        unknown = set(given) - set(defaults)
        if unknown:
            raise ValueError("%s: unknown keys %s" % (name, sorted(unknown)))
        defaults.update(given)
    return defaults


# What train= configures, by the Stepper's prefix of the trainer's entry points: the option whose head
# the trainer needs and the refusal's text when it, network= or memory= is missing, the trainer's
# settings (aigar_amd.net), and for a trainer with a critic its spec from `parameters`, the critic's
# input length (what a critic= spec without n_in gets) and the Stepper's configuration method.
_Trainer = collections.namedtuple("_Trainer", "needs refusal settings critic_spec critic_n_in critic_config")
_TRAINERS = {
    "train": _Trainer("discrete",
                      "train= needs discrete=, network= and memory= (Q-learning on the device's replay memory)",
                      _net.train_params, None, None, None),
    "actrain": _Trainer("continuous",
                        "train= with continuous= needs network= and memory= (CACLA on the device's replay memory)",
                        _net.actrain_params, lambda p, n_in, n_act: _net.critic_spec(p, n_in=n_in),
                        lambda n_in, n_act: n_in, "critic_config"),
    "dpg": _Trainer("continuous",
                    "train='dpg' needs continuous=, network= and memory= (DPG on the device's replay memory)",
                    _net.dpg_params, lambda p, n_in, n_act: _net.qcritic_spec(p, n_in=n_in, n_act=n_act),
                    lambda n_in, n_act: n_in + n_act, "qcritic_config"),
    "spg": _Trainer("continuous",
                    "search= needs train='dpg', continuous=, network= and memory= (SPG on the DPG trainer's critic)",
                    _net.spg_params, lambda p, n_in, n_act: _net.qcritic_spec(p, n_in=n_in, n_act=n_act),
                    lambda n_in, n_act: n_in + n_act, "qcritic_config"),
}
_SEARCH_KEYS = ("samples", "moving", "replace", "prio_evals", "fused", "noise", "noise_decay", "seed")


class AgarVecEnv:
    def __init__(self, n_players, parameters=None, n_arenas=1, virus=None, field_size=0, max_pellets=-1.0,
                 max_viruses=-1.0, device=0, torch_stream=True, roles=None, reset_limit=None, desync=True, seed=0,
                 score=False, pixels=None, pixel_dtype=None, memory=None, discrete=None, continuous=None, network=None,
                 train=None, critic=None):
        import torch
        if continuous and discrete:
            raise ValueError("continuous= and discrete= exclude each other (one learner decides per env)")
        self.torch = torch
        self.parameters = parameters
        g = (lambda n, dflt: getattr(parameters, n, dflt)) if parameters is not None else (lambda n, dflt: dflt)
        self._g = g  # (a setting of `parameters`, or the given default)
        ch, ex, gsq = obs_masks(parameters)
        virus = bool(g("VIRUS_SPAWN", False)) if virus is None else bool(virus)
        if not virus:
            ch &= ~_abi.OBS_VIRUS
        c = _abi.Config()
        c.n_arenas, c.bots_per_arena, c.field_size = n_arenas, n_players, field_size
        c.virus_enabled = int(virus)
        c.max_pellets, c.max_viruses = float(max_pellets), float(max_viruses)
        c.grid_squares, c.obs_channels, c.obs_extras = gsq, ch, ex
        c.rng_mode, c.device = _abi.RNG_PHILOX, device
        if score:
            c.flags |= _abi.FLAG_SCORE
        self.stepper = Stepper(c)
        self.dev = torch.device("cuda", device)
        if torch_stream:
            self.stepper.set_stream(torch.cuda.current_stream(self.dev).cuda_stream)
        self.NP, self.A, self.B = self.stepper.NP, n_arenas, n_players
        self.skip = int(g("FRAME_SKIP_RATE", 0))
        self.enable_split = bool(g("ENABLE_SPLIT", False))
        self.reward_params = _abi.RewardParams.from_parameters(parameters)
        self.seed = int(seed)
        # roles: per player of one arena (repeated in every arena) or of all arenas
        if roles is None:
            roles = ["NN"] * n_players
        roles = [_abi.ROLES[r] if isinstance(r, str) else int(r) for r in roles]
        if len(roles) == n_players:
            roles = roles * n_arenas
        if len(roles) != self.NP:
            raise ValueError("roles: %d entries for %d players per arena x %d arenas" % (len(roles), n_players,
                                                                                          n_arenas))
        self.roles = np.array(roles, np.uint8)
        self.stepper.set_roles(self.roles)
        self.stepper.env_config(greedy_split=bool(g("ENABLE_GREEDY_SPLIT", False)), random_skip=max(1, self.skip),
                                random_split=self.enable_split, random_eject=bool(g("ENABLE_EJECT", False)),
                                salt=self.seed)
        self.nn = torch.as_tensor(self.roles == _abi.ROLE_NN, device=self.dev)
        self._nn_u8 = self.nn.to(torch.uint8)
        self._mixed = bool((self.roles != _abi.ROLE_NN).any())
        # the other bots' policies (step_calls and the warm-up move them call by call)
        self._greedy = torch.as_tensor(self.roles == _abi.ROLE_GREEDY, device=self.dev).to(torch.uint8)
        self._has_greedy = bool((self.roles == _abi.ROLE_GREEDY).any())
        self._has_random = bool((self.roles == _abi.ROLE_RANDOM).any())
        self._greedy_split = bool(g("ENABLE_GREEDY_SPLIT", False))
        self.reset_limit = int(g("RESET_LIMIT", 20000) if reset_limit is None else reset_limit)
        self.desync = bool(desync) and self.reset_limit > 0 and n_arenas > 1
        self.age = np.zeros(n_arenas, np.int64)
        self._resets = 0
        self.pixels = tuple(pixels) if pixels is not None else pixel_params(parameters)
        if self.pixels is not None:
            side, rgb, last = self.pixels
            self.stepper.pixel_config(side, rgb=rgb, last=last, color_seed=self.seed)
            self.obs = torch.empty(self.stepper.pixel_state_shape, dtype=pixel_dtype or torch.float32, device=self.dev)
        else:
            self.obs = torch.empty((self.NP, self.stepper.obs_len), dtype=torch.float64, device=self.dev)
        self._mask = torch.zeros(self.NP, dtype=torch.uint8, device=self.dev)  # (persistent: read on the stepper's stream)
        self._r = torch.empty(self.NP, dtype=torch.float64, device=self.dev)
        self._act = {}  # n_act -> persistent action buffer (the decision graph is keyed by its address)
        self._own_stream = not torch_stream  # (the stepper's work is then not ordered with torch's)
        self._scored = bool(score)
        if self._scored:
            self._score = torch.empty((self.NP, 4), dtype=torch.float64, device=self.dev)
            self._ret = torch.zeros(self.NP, dtype=torch.float64, device=self.dev)
            nan = float("nan")
            # the last finished episode of every arena: NaN until its first episode has ended
            self.last_score = torch.full((self.NP, 4), nan, dtype=torch.float64, device=self.dev)
            self.last_return = torch.full((self.NP,), nan, dtype=torch.float64, device=self.dev)
        self._setup_memory(memory, continuous)
        self._setup_selection(discrete)
        self._setup_noise(continuous)
        self._setup_network(network)
        self._setup_trainer(train, critic, self._search_option())

    def _search_option(self):
        """The search= option of the trainer (None here: the keyword is AgarSpgEnv's)."""
        return None

    def _setup_memory(self, memory, continuous):
        g = self._g
        self.memory = None
        if memory:  # (explicit only: existing callers pass full parameter sets)
            m = _settings("memory", {"capacity": int(g("MEMORY_CAPACITY", 40000)),
                                     "prioritized": bool(g("PRIORITIZED_EXP_REPLAY_ENABLED", False)),
                                     "alpha": float(g("MEMORY_ALPHA", 0.6)), "beta": float(g("MEMORY_BETA", 0.4)),
                                     "batch": int(g("MEMORY_BATCH_LEN", 32)), "seed": self.seed}, memory)
            self.memory = m
            self.stepper.exp_config(m["capacity"], prioritized=m["prioritized"], alpha=m["alpha"], beta=m["beta"],
                                    dtype=self.obs.dtype, seed=m["seed"], extra=bool(continuous))

    def _setup_selection(self, discrete):
        torch, g = self.torch, self._g
        self.discrete = None
        if discrete:  # (explicit only, as memory=)
            dd = _settings("discrete", {"num_actions": int(g("NUM_ACTIONS", 25)),
                                        "square": bool(g("SQUARE_ACTIONS", True)),
                                        "strategy": g("EXPLORATION_STRATEGY", "e-Greedy"), "seed": self.seed}, discrete)
            if dd["strategy"] not in _abi.STRATEGIES:
                raise ValueError("discrete: strategy must be one of %s" % sorted(_abi.STRATEGIES))
            self._table = _actions.discrete_actions(dd["num_actions"], dd["square"], self.enable_split,
                                                    bool(g("ENABLE_EJECT", False)))
            dd["n_out"] = int(self._table.shape[0])
            self.discrete = dd
            self.actions = torch.as_tensor(self._table, device=self.dev)
            self.explore = torch.tensor([float(g("EPSILON", 0.0)), float(g("TEMPERATURE", 0.0))], dtype=torch.float64,
                                        device=self.dev)
            self._q = {}  # dtype -> persistent Q buffer (the decision graph is keyed by its address)
            self._u = torch.empty((self.NP, 3), dtype=torch.float64, device=self.dev)
            self._idx = torch.empty(self.NP, dtype=torch.int32, device=self.dev)
            self._val = torch.empty(self.NP, dtype=torch.float64, device=self.dev)
            self.action_idx = self.action_value = None
            self._act_q = torch.zeros((self.NP, 4), dtype=torch.float64, device=self.dev)  # step_q_calls' chosen rows
            self._q_dtype = None
            self._decide_dtype(torch.float32)

    def _setup_noise(self, continuous):
        torch, g = self.torch, self._g
        self.continuous = None
        if continuous:  # (explicit only, as memory=)
            cc = _settings("continuous", {"noise": g("NOISE_TYPE", "Gaussian"),
                                          "theta": float(g("ORN_UHL_THETA", 0.15)),
                                          "mu": float(g("ORN_UHL_MU", 0)), "dt": float(g("ORN_UHL_DT", 0.01)),
                                          "std": float(g("GAUSSIAN_NOISE", 1.0)),
                                          "store_raw": g("ALGORITHM", "CACLA") == "CACLA" and not self._search_option(),
                                          "seed": self.seed},
                            continuous)
            if cc["noise"] not in _abi.NOISE_TYPES:
                raise ValueError("continuous: noise must be one of %s" % sorted(_abi.NOISE_TYPES))
            cc["n_act"] = 2 + int(self.enable_split) + int(bool(g("ENABLE_EJECT", False)))
            self.continuous = cc
            self.noise_std = torch.tensor([cc["std"]], dtype=torch.float64, device=self.dev)
            # the persistent actor-output buffer (the decision graph is keyed by its address): always
            # float64, so a float32 mu is widened exactly by the copy into it and the handle's noise
            # is configured once, here -- no call reconfigures it (that would restart the Orn-Uhl
            # state and drop the captured graph)
            self._mu = torch.empty((self.NP, cc["n_act"]), dtype=torch.float64, device=self.dev)
            self._nu = {}  # T -> persistent draw buffer
            self._noisy = torch.empty((self.NP, cc["n_act"]), dtype=torch.float64, device=self.dev)
            self.noisy_action = None
            # step_ac_calls' twin of the handle's buffers: the held rows and the Orn-Uhl state
            self._act_ac = torch.zeros((self.NP, cc["n_act"]), dtype=torch.float64, device=self.dev)
            self._ou_ac = torch.zeros((self.NP, cc["n_act"]), dtype=torch.float64, device=self.dev)
            self.stepper.noise_config(cc["n_act"], cc["noise"], torch.float64, theta=cc["theta"], ou_mu=cc["mu"],
                                      dt=cc["dt"], seed=cc["seed"], store_raw=cc["store_raw"])

    def _setup_network(self, network):
        torch, parameters = self.torch, self.parameters
        self.network = None
        self._obs_ready = False  # (`obs` holds the current states: what step_net's network reads)
        if network:  # (explicit only, as memory=)
            if self.discrete is None and self.continuous is None:
                raise ValueError("network= needs discrete= or continuous= (the head that follows the network)")
            head = "q" if self.discrete is not None else "actor"
            n_out = self.discrete["n_out"] if self.discrete is not None else self.continuous["n_act"]
            n_in = int(self.stepper.obs_len)
            if self.pixels is not None:  # the CNN learner: conv layers on the pixel state
                if network is True:
                    spec = _net.cnn_spec(parameters, head, n_out=n_out)
                elif hasattr(network, "convs") or len(network) == len(_net.CnnSpec._fields):
                    spec = _net.CnnSpec(*network)
                else:
                    raise ValueError("network=: the device network takes no pixel state without a conv part "
                                     "(a CnnSpec, aigar_amd.net.cnn_spec)")
                side, channels = self.stepper.pixel_state_shape[1], self.stepper.pixel_state_shape[3]
                if (spec.side, spec.channels) != (side, channels):
                    raise ValueError("network=: the conv part takes images %d x %d x %d, the env's pixel state is "
                                     "%d x %d x %d" % (spec.side, spec.side, spec.channels, side, side, channels))
                if spec.units[-1] != n_out:
                    raise ValueError("network=: %d outputs, the env has a head of %d" % (spec.units[-1], n_out))
            else:
                if network is True:
                    spec = _net.mlp_spec(parameters, head, n_in=n_in, n_out=n_out)
                elif hasattr(network, "convs"):
                    raise ValueError("network=: a CnnSpec needs a pixel state (pixels=)")
                else:
                    spec = _net.NetSpec(*network)
                    if spec.n_in is None:
                        spec = spec._replace(n_in=n_in)
                if spec.n_in != n_in or spec.units[-1] != n_out:
                    raise ValueError("network=: %d inputs and %d outputs, the env has states of %d values and a head "
                                     "of %d" % (spec.n_in, spec.units[-1], n_in, n_out))
            self.network = spec
            self._head = head
            self.stepper.net_config(spec, self.obs.dtype)
            if self.discrete is not None:
                self._decide_dtype(torch.float64)  # (the network's output buffer is float64)
            self._net_out = torch.empty((self.NP, n_out), dtype=torch.float64, device=self.dev)
            self.net_output = None

    def _setup_trainer(self, train, critic, search=None):
        parameters = self.parameters
        self.training = None
        self._trainer = None  # the Stepper's trainer family that train= configured: "train", "actrain", "dpg" or "spg"
        self.critic = None
        if critic is not None and not (train and self.continuous is not None):
            raise ValueError("critic= needs continuous= and train= (the CACLA or DPG trainer's critic)")
        dpg = train == "dpg" or (isinstance(train, dict) and str(train.get("algorithm", "")).lower() == "dpg")
        if isinstance(train, str) and not dpg:
            raise ValueError("train=%r: True, a dict or 'dpg'" % (train,))
        if isinstance(train, dict) and "algorithm" in train and not dpg:
            raise ValueError("train: algorithm = %r: 'dpg' (the other trainers follow from discrete= / continuous=)"
                             % (train["algorithm"],))
        kind = "dpg" if dpg else "actrain" if self.continuous is not None else "train"
        if search:
            if not dpg:
                raise ValueError("search= needs train='dpg' or train=dict(algorithm='dpg', ...) (SPG searches on the DPG "
                                 "trainer's critic)")
            kind = "spg"
        if train:  # (explicit only, as memory=)
            row = _TRAINERS[kind]
            if getattr(self, row.needs) is None or self.network is None or self.memory is None:
                raise ValueError(row.refusal)
            cnn = self.pixels is not None or hasattr(self.network, "convs")
            if cnn and kind != "train":  # (Q-learning alone trains a conv part: DESIGN.md §4p)
                raise ValueError("train=: CNN / pixel states are not trained on the device")
            # the trainer's settings: the parameters' own with the memory's batch, then the
            # overrides of a train= dict, whose "algorithm" key is no setting
            # (the CNN Q-learner: CNN_REPR is what train_params refuses for the other settings' sake)
            tp = row.settings(_net._Dense(parameters) if cnn and parameters is not None else parameters)
            tp["batch"] = int(self.memory["batch"])
            if isinstance(train, dict):
                own = {k: v for k, v in train.items() if k != "algorithm"}
                if kind == "spg":  # (the search's settings are search='s, not train='s; it has no q_increase)
                    if "q_increase" in own:
                        raise ValueError("train: q_increase = %r: the SPG step has no Q-value increase (search=)"
                                         % (own["q_increase"],))
                    tp = dict(_settings("train", {k: v for k, v in tp.items() if k not in _SEARCH_KEYS}, own),
                              **{k: tp[k] for k in _SEARCH_KEYS})
                else:
                    tp = _settings("train", tp, own)
            if kind == "spg":
                tp["seed"] = self.seed
                if not isinstance(search, dict):
                    search = {}
                tp.update(_settings("search", {k: tp[k] for k in _SEARCH_KEYS}, search))
            if row.critic_spec is not None:
                n_in, n_act = int(self.stepper.obs_len), int(self.network.units[-1])
                cs = row.critic_spec(parameters, n_in, n_act) if critic is None else _net.NetSpec(*critic)
                if cs.n_in is None:
                    cs = cs._replace(n_in=row.critic_n_in(n_in, n_act))
                self.critic = cs
                getattr(self.stepper, row.critic_config)(cs, self.obs.dtype)
            self.training, self._trainer = tp, kind
            getattr(self.stepper, kind + ("_config_cnn" if cnn else "_config"))(**tp)
        self.cacla = self._trainer == "actrain"  # (the trainer is the CACLA learner's: DESIGN.md §4m)
        self.dpg = self._trainer == "dpg"  # (... the DPG learner's: §4n)
        self.spg = self._trainer == "spg"  # (... the SPG learner's, on the DPG learner's critic: §4o)

    def _ordered(self, call, *args, **kw):
        """A stepper call outside the decision that reads or writes torch's tensors.  On torch's
        stream it is ordered like any kernel.  A stepper with its own stream is ordered here:
        what torch has queued (the arguments) is finished before the call, and the call's work
        before it returns -- so the results are there for torch, and the arguments may be freed."""
        if self._own_stream:
            self.torch.cuda.synchronize(self.dev)
        out = call(*args, **kw)
        if self._own_stream:
            self.stepper.sync()
        return out

    def _need_network(self):
        if self.network is None:
            raise RuntimeError("AgarVecEnv was created without network=")

    # ---- the Q-learning trainer on the device
    def _need_training(self):
        if self.training is None:
            raise RuntimeError("AgarVecEnv was created without train=")

    def train(self, n=1, u=None):
        """n training steps of the acting network on the replay memory, one graph replay each with
        no host work in between: draw, forward, TD errors, priorities, backward, Adam in place,
        target copy when due.  u: None (the memory's own stream) or [n, batch] draws in [0, 1).
        A step is skipped on the device while the memory is too small (train_info)."""
        self._need_training()
        torch = self.torch
        n = int(n)
        if n < 1:
            raise ValueError("train: n must be at least 1")
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float64, device=self.dev).reshape(n, self.training["batch"]).contiguous()
        self._ordered(getattr(self.stepper, self._trainer + "_step"), n, u)  # (u is freed when this returns)

    def sync_target(self):
        """The trainer's target network(s) <- the online one(s) now (aigar_*_sync_target)."""
        self._need_training()
        self._ordered(getattr(self.stepper, self._trainer + "_sync_target"))

    def train_info(self):
        """{steps, skipped, since_target} (aigar_train_info: a host round trip); the CACLA trainer's
        also has actor_epochs, selected, epochs, cut and epochs_skipped (aigar_actrain_info), the
        DPG trainer's actor_steps and actor_skipped (aigar_dpg_info)."""
        self._need_training()
        return getattr(self.stepper, self._trainer + "_info")()

    def train_td(self):
        """(td [batch] float64, idx [batch] int64) of the last drawn training step, device tensors."""
        self._need_training()
        torch = self.torch
        b = self.training["batch"]
        td = torch.empty(b, dtype=torch.float64, device=self.dev)
        idx = torch.empty(b, dtype=torch.int64, device=self.dev)
        self._ordered(getattr(self.stepper, self._trainer + "_td"), td, idx)
        return td, idx

    def get_weights(self, target=False):
        """The acting network's dense weights as [(W [in, out], b [out])] float32 numpy arrays
        (Keras' layout; aigar_amd.net.weights_to_torch loads them into a module); target=True:
        the trainer's target network.  With a conv part its pairs (W [k, k, Cin, F], b [F]) come
        first (aigar_amd.net.cnn_weights_to_torch loads the list into a module)."""
        self._need_network()
        if target:
            self._need_training()
        return self._ordered(self.stepper.net_get_weights, "target" if target else "online")

    # ---- the CACLA learner's critic and the DPG learner's (§4n)
    def _need_cacla(self):
        if not self.cacla:
            raise RuntimeError("AgarVecEnv was created without continuous= and train= (the CACLA trainer)")

    def _need_critic(self):
        if not (self.cacla or self.dpg or self.spg):
            raise RuntimeError("AgarVecEnv was created without continuous= and train= (the CACLA or DPG trainer)")

    def set_critic_weights(self, weights):
        """The critic's weights, as set_weights takes the acting network's.  The trainer's target
        keeps what it holds (train= copied the critic as it was then)."""
        self._need_critic()
        self._push_weights(weights, _net.weights_from_torch, self.stepper.critic_set_weights)

    def get_critic_weights(self, target=False):
        """The critic's (target=True: its target's) weights as [(W [in, out], b [out])] float32 numpy arrays."""
        self._need_critic()
        return self._ordered(self.stepper.critic_get_weights, "target" if target else "online")

    def critic_value(self, states):
        """V(s) of states [rows, n_in] (a device tensor or an array) -> [rows] float64 device tensor."""
        self._need_cacla()
        return self._critic_rows(self._float_states(states))

    def _float_states(self, states):
        """states as a device tensor, float64 unless they are float32."""
        torch = self.torch
        x = torch.as_tensor(states, device=self.dev)
        if x.dtype not in (torch.float64, torch.float32):
            x = x.to(torch.float64)
        return x

    def _critic_rows(self, x):
        """The critic on its input rows x [rows, critic n_in] -> [rows] float64 device tensor."""
        x = x.contiguous()
        out = self.torch.empty(x.shape[0], dtype=self.torch.float64, device=self.dev)
        self._ordered(self.stepper.critic_forward, x, out)
        return out

    def q_value(self, states, actions):
        """Q(s, a) of states [rows, n_in] and actions [rows, n_act] (device tensors or arrays) with
        the DPG trainer's critic -> [rows] float64 device tensor.  The row [s, a] is built in the
        states' dtype (float64 unless they are float32)."""
        if not (self.dpg or self.spg):
            raise RuntimeError("AgarVecEnv was created without train='dpg' (the DPG trainer)")
        torch = self.torch
        s = self._float_states(states)
        a = torch.as_tensor(actions, device=self.dev).to(s.dtype)
        n_act = self.critic.n_in - int(self.stepper.obs_len)
        if s.ndim != 2 or a.ndim != 2 or a.shape[0] != s.shape[0] or a.shape[1] != n_act:
            raise ValueError("q_value: states [rows, n_in] and actions [rows, %d], got %s and %s"
                             % (n_act, tuple(s.shape), tuple(a.shape)))
        return self._critic_rows(torch.cat([s, a], dim=1))

    def cacla_var(self):
        """CACLA-Var's running variance of the TD error (a host round trip)."""
        self._need_cacla()
        return self.stepper.actrain_var()

    def set_weights(self, weights):
        """The trainer's weight push: a list of (W [in, out], b [out]) float32 per layer as device
        tensors or arrays, or anything aigar_amd.net.weights_from_torch takes (a torch module or
        state dict of nn.Linear layers, a flat Keras-layout list; with a conv part the conv
        pairs (W [k, k, Cin, F], b [F]) first, aigar_amd.net.cnn_weights_from_torch).  Takes
        effect at the next decision; the captured graph stays."""
        self._need_network()
        if hasattr(self.network, "convs"):
            convert = lambda w: _net.cnn_weights_from_torch(w, self.network)
        else:
            convert = _net.weights_from_torch
        self._push_weights(weights, convert, self.stepper.net_set_weights)

    def _push_weights(self, weights, convert, push):
        """weights through push (the Stepper's net_set_weights or critic_set_weights): pairs of
        device tensors go as float32 device tensors, anything else through convert."""
        torch = self.torch
        pairs = isinstance(weights, (list, tuple)) and all(
            isinstance(p, (list, tuple)) and len(p) == 2 and isinstance(p[0], torch.Tensor) and p[0].is_cuda
            for p in weights)
        if pairs:
            ws = [(W.to(torch.float32).contiguous(), b.to(device=self.dev, dtype=torch.float32).contiguous())
                  for W, b in weights]
        else:
            ws = convert(weights)
        self._ordered(push, ws)  # (ws is freed when this returns)

    def _net_decisions(self, n, u=None):
        """n decisions with the network in front, one graph replay each, no host work between."""
        torch = self.torch
        self._need_network()
        if not self._obs_ready:
            raise RuntimeError("step_net: `obs` does not hold the current states yet: call reset() or observe() first")
        kw = dict(enable_split=self.enable_split, skip=self.skip, params=self.reward_params, n_decisions=n)
        if self._head == "q":
            u = self._q_draws(u)
            self._decide_dtype(torch.float64)
            self.stepper.env_step_net("q", self.explore, self._r, self.obs, idx=self._idx, val=self._val, u=u, **kw)
            self.action_idx, self.action_value = self._idx.clone(), self._val.clone()
        else:
            u = self._noise_draws(u, "step_net")
            self.stepper.env_step_net("actor", self.noise_std, self._r, self.obs, u=u, noisy=self._noisy, **kw)
            self.noisy_action = self._noisy.clone()
        self.stepper.net_output(self._net_out)
        self.net_output = self._net_out.clone()

    def step_net(self, u=None):
        """One decision with the acting network on the device: the network on `obs`, then the
        selection (as `step_q`; u [n_players, 3]) or the noise (as `step_ac`; u [n_players, 2,
        T, 2]) and the decision, one graph replay -> (obs, reward, alive, done).  Leaves
        `net_output` (the Q values or mu; rows of dead and non-NN players keep what they held)
        and `action_idx` / `action_value` or `noisy_action` fresh."""
        self._net_decisions(1, u)
        return self._after_decision()

    def _run_length(self, left):
        """Decisions until (and with) the next one that ends an episode, at most left."""
        if self._scored:
            return 1  # (the episode returns add every decision's reward on the torch side)
        if self.reset_limit <= 0:
            return left
        per = self.skip + 1
        room = (self.reset_limit - self.skip + 2) - self.age  # (over: age > limit - skip + 2)
        need = int(np.min(np.maximum(room, 0) // per)) + 1
        return max(1, min(left, need))

    def collect(self, n):
        """n decisions as `step_net()` makes them, with no Python between the graph replays of a
        run: the runs are split where an arena's episode ends (the arenas' ages are host-side, so
        the split points are known without a sync), and the ended arenas are reset between runs.
        The device (worlds, memory, scores, `obs`, Orn-Uhl states) is left exactly as n calls of
        `step_net()` leave it.  Returns the last decision's (obs, reward, alive, done), done
        OR-ed over the n decisions.  With score=True every decision is a run of its own."""
        self._need_network()
        n = int(n)
        if n < 1:
            raise ValueError("collect: n must be at least 1")
        done_any = None
        out = None
        left = n
        while left:
            r = self._run_length(left)
            self._net_decisions(r)
            if self.reset_limit > 0:
                self.age += (r - 1) * (self.skip + 1)  # (_after_decision adds the last one's)
            out = self._after_decision()
            done_any = out[3] if done_any is None else done_any | out[3]
            left -= r
        return out[0], out[1], out[2], done_any

    def _need_continuous(self):
        if self.continuous is None:
            raise RuntimeError("AgarVecEnv was created without continuous=")

    def set_noise(self, std):
        """Write the decision's noise level (the device tensor `noise_std`)."""
        self._need_continuous()
        self.noise_std[0] = float(std)

    def _mu_buffers(self, mu, u, what):
        torch = self.torch
        self._need_continuous()
        n = self.continuous["n_act"]
        if not isinstance(mu, torch.Tensor):
            mu = torch.as_tensor(np.asarray(mu), device=self.dev)
        if mu.dtype not in (torch.float32, torch.float64):
            raise ValueError("%s: mu must be float32 or float64, got %s" % (what, mu.dtype))
        if tuple(mu.shape) != (self.NP, n):
            raise ValueError("%s: mu must be [%d, %d], got %s" % (what, self.NP, n, tuple(mu.shape)))
        buf = self._mu
        buf.copy_(mu)  # (float32 -> float64: exact)
        return buf, self._noise_draws(u, what)

    def _noise_draws(self, u, what):
        """The decision's given draws u [NP, 2, T, 2] in the persistent buffer of their T (the
        decision graph is keyed by its address); None (the device's own) stays None."""
        if u is None:
            return None
        torch = self.torch
        u = torch.as_tensor(u, dtype=torch.float64, device=self.dev)
        if u.dim() != 4 or tuple(u.shape[:2]) != (self.NP, 2) or int(u.shape[3]) != 2:
            raise ValueError("%s: u must be [%d, 2, T, 2], got %s" % (what, self.NP, tuple(u.shape)))
        ub = self._nu.get(int(u.shape[2]))
        if ub is None:
            ub = self._nu[int(u.shape[2])] = torch.empty(tuple(u.shape), dtype=torch.float64, device=self.dev)
        ub.copy_(u)
        return ub

    def step_ac(self, mu, u=None):
        """mu: [n_players, n_act] float32 / float64 device tensor of the actor's outputs (rows of
        dead and non-NN players are ignored; float32 is widened exactly, and either dtype may
        follow the other) -> (obs, reward, alive, done) as `step`; the noise and the decision
        are one graph replay.  u: [n_players, 2, T, 2] uniforms in [0, 1) (row,
        pair, attempt, {ua, ub}; T <= 16), None: the device's own.  Leaves a fresh clone of the
        noisy actions in `noisy_action` (NaN rows where nobody decided)."""
        buf, u = self._mu_buffers(mu, u, "step_ac")
        self.stepper.env_step_ac(buf, self.noise_std, self._r, self.obs, u=u, noisy=self._noisy,
                                 enable_split=self.enable_split, skip=self.skip, params=self.reward_params)
        self.noisy_action = self._noisy.clone()
        return self._after_decision()

    def step_ac_calls(self, mu, u=None):
        """The same decision as separate calls (noise, then `step_calls`); without the episode
        bookkeeping and the replay memory's fifth field.  This path keeps its own Orn-Uhl state
        (`_ou_ac`), cleared by `reset` and at an episode's end, not by direct stepper calls."""
        torch = self.torch
        buf, u = self._mu_buffers(mu, u, "step_ac_calls")
        # who decides: the live NN players, as the kernel tests it
        alive = self.stepper.player_stats()[:, 0] != 0
        deciding = torch.as_tensor(alive, device=self.dev) & self.nn
        ou = self._ou_ac.clone()
        out = torch.empty_like(self._noisy)
        self.stepper.noise(buf, self.noise_std, out, u=u, prev=ou if self.stepper.noi[2] else None)
        d2 = deciding[:, None]
        self._ou_ac = torch.where(d2, ou, self._ou_ac)
        self._act_ac = torch.where(d2, out, self._act_ac)
        self.noisy_action = torch.where(d2, out, torch.full_like(out, float("nan")))
        return self.step_calls(self._act_ac)

    def perturb(self, actions, std=None, u=None, prev=None):
        """The noise alone (aigar_noise) on any rows: actions [rows, n_act] float32 / float64 ->
        a fresh float64 tensor of noisy actions.  std: a float or a [1] float64 device tensor
        (None: `noise_std`); u: [rows, 2, T, 2] uniforms (None: the device's own); prev: the
        caller's [rows, n_act] float64 Orn-Uhl state, advanced in place (needed for Orn-Uhl).
        Liveness and roles are ignored, and nothing of the decision is touched: not the players'
        Orn-Uhl state, not the captured graph.  The device's own draws depend on (row, pair,
        attempt, tick, seed) alone: a second call before the next decision gives row r the same
        normals, and so does the decision itself for rows below n_players -- pass u, or put the
        batches into one call as further rows."""
        torch = self.torch
        self._need_continuous()
        a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions), device=self.dev)
        if a.dtype not in (torch.float32, torch.float64):
            raise ValueError("perturb: actions must be float32 or float64, got %s" % a.dtype)
        if a.dim() != 2 or int(a.shape[1]) != self.continuous["n_act"]:
            raise ValueError("perturb: actions must be [rows, %d], got %s" % (self.continuous["n_act"], tuple(a.shape)))
        a = a.to(device=self.dev, dtype=torch.float64).contiguous()  # (float32 -> float64: exact)
        if std is None:
            std = self.noise_std
        elif not isinstance(std, torch.Tensor):
            std = torch.tensor([float(std)], dtype=torch.float64, device=self.dev)
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float64, device=self.dev).contiguous()
        out = torch.empty(tuple(a.shape), dtype=torch.float64, device=self.dev)
        self._ordered(self.stepper.noise, a, std, out, u=u, prev=prev)
        return out

    def sample_extra(self, idx):
        """(extra [batch, 4] float64, valid [batch] bool) of the memory slots idx: the tuple's
        fifth field -- CACLA's raw action, or what `update_actions` wrote; NaN and False where
        the slot has none (the reference's None) or idx is outside [0, size)."""
        if self.memory is None or self.continuous is None:
            raise RuntimeError("AgarVecEnv was created without memory= and continuous=")
        torch = self.torch
        idx = torch.as_tensor(idx, dtype=torch.int64, device=self.dev).contiguous()
        extra = torch.full((int(idx.shape[0]), 4), float("nan"), dtype=torch.float64, device=self.dev)
        valid = torch.zeros(int(idx.shape[0]), dtype=torch.bool, device=self.dev)
        self._ordered(self.stepper.exp_extra_get, idx, extra, valid)
        return extra, valid

    def update_actions(self, idx, actions):
        """The trainer's write-back of the best sampled actions (aigar.py:1079-1086,
        replay_buffer.py update_dones): slot idx[j] gets actions[j] ([n, n_act] or [n, 4],
        padded with zeros) as its fifth field; the last of a repeated index wins."""
        if self.memory is None or self.continuous is None:
            raise RuntimeError("AgarVecEnv was created without memory= and continuous=")
        torch = self.torch
        idx = torch.as_tensor(idx, dtype=torch.int64, device=self.dev).contiguous()
        a = torch.as_tensor(actions, dtype=torch.float64, device=self.dev)
        rows = torch.zeros((int(idx.shape[0]), 4), dtype=torch.float64, device=self.dev)
        rows[:, :a.shape[1]] = a
        self._ordered(self.stepper.exp_extra_set, idx, rows)  # (rows is freed when this returns)

    def _decide_dtype(self, dtype):
        """(Re)configure the selection for Q rows of dtype (the kernel is built per dtype)."""
        if dtype is not self._q_dtype:
            self.stepper.decide_config(self._table, self.discrete["strategy"], dtype, self.discrete["seed"])
            self._q_dtype = dtype

    def set_exploration(self, epsilon=None, temperature=None):
        """Write the decision's epsilon and / or temperature (the device tensor `explore`)."""
        self._need_discrete()
        if epsilon is not None:
            self.explore[0] = float(epsilon)
        if temperature is not None:
            self.explore[1] = float(temperature)

    def _need_discrete(self):
        if self.discrete is None:
            raise RuntimeError("AgarVecEnv was created without discrete=")

    def _q_buffers(self, q, u):
        torch = self.torch
        self._need_discrete()
        if not isinstance(q, torch.Tensor):
            q = torch.as_tensor(np.asarray(q), device=self.dev)
        if q.dtype not in (torch.float32, torch.float64):
            raise ValueError("step_q: q must be float32 or float64, got %s" % q.dtype)
        if tuple(q.shape) != (self.NP, self.discrete["n_out"]):
            raise ValueError("step_q: q must be [%d, %d], got %s" % (self.NP, self.discrete["n_out"], tuple(q.shape)))
        buf = self._q.get(q.dtype)
        if buf is None:
            buf = self._q[q.dtype] = torch.empty((self.NP, self.discrete["n_out"]), dtype=q.dtype, device=self.dev)
        buf.copy_(q)
        self._decide_dtype(q.dtype)
        return buf, self._q_draws(u)

    def _q_draws(self, u):
        """The selection's given draws u [NP, 3] in their persistent buffer; None stays None."""
        if u is not None:
            self._u.copy_(self.torch.as_tensor(u, dtype=self.torch.float64, device=self.dev))
            u = self._u
        return u

    def step_q(self, q, u=None):
        """q: [n_players, n_out] float32 / float64 device tensor of action values (rows of
        dead and non-NN players are ignored) -> (obs, reward, alive, done) as `step`; the
        selection and the decision are one graph replay.  u: [n_players, 3] draws in [0, 1)
        (coin, explore index, Boltzmann draw), None: the device's own.  Leaves fresh clones in
        `action_idx` (int32, -1 where nobody decided) and `action_value`."""
        buf, u = self._q_buffers(q, u)
        self.stepper.env_step_q(buf, self.explore, self._r, self.obs, self._idx, self._val, u=u,
                                enable_split=self.enable_split, skip=self.skip, params=self.reward_params)
        self.action_idx, self.action_value = self._idx.clone(), self._val.clone()
        return self._after_decision()

    def step_q_calls(self, q, u=None):
        """The same decision as separate calls (decide, then `step_calls`); without the
        episode bookkeeping."""
        buf, u = self._q_buffers(q, u)
        # (persistent, as the handle's own buffer in step_q: a player that does not decide
        # keeps its last chosen row, and moves by it if it respawns on a skipped tick)
        self.stepper.decide(buf, self.explore, self._idx, self._val, u=u, act=self._act_q)
        self.action_idx, self.action_value = self._idx.clone(), self._val.clone()
        return self.step_calls(self._act_q)

    def sample(self, batch=None, u=None):
        """One mini-batch of the replay memory as device tensors (s, a, r, s2, done, w, idx):
        batch draws (MEMORY_BATCH_LEN by default), from the float64 tensor u [batch] in [0, 1)
        or the memory's own stream.  w are the importance weights (1.0 in uniform mode).  A
        memory too small to draw from gives idx -1 and w NaN (rows zero)."""
        if self.memory is None:
            raise RuntimeError("AgarVecEnv was created without memory=")
        torch = self.torch
        n = int(self.memory["batch"] if batch is None else batch)
        row = tuple(self.obs.shape[1:])
        s = torch.zeros((n,) + row, dtype=self.obs.dtype, device=self.dev)
        s2 = torch.zeros_like(s)
        a = torch.zeros((n, 4), dtype=torch.float64, device=self.dev)
        r = torch.zeros(n, dtype=torch.float64, device=self.dev)
        done = torch.zeros(n, dtype=torch.bool, device=self.dev)
        w = torch.empty(n, dtype=torch.float64, device=self.dev)
        idx = torch.empty(n, dtype=torch.int64, device=self.dev)
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float64, device=self.dev).contiguous()
        self._ordered(self.stepper.exp_sample, w, idx, u=u, s=s, a=a, r=r, s2=s2, done=done)
        return Batch(s, a, r, s2, done, w, idx)

    def update_priorities(self, idx, td_error):
        """The trainer's write-back (aigar.py:1075-1086): priority |td_error| + 1e-4 for the
        sampled idx; nothing in uniform mode (ReplayBuffer.update_priorities)."""
        if self.memory is None:
            raise RuntimeError("AgarVecEnv was created without memory=")
        if not self.memory["prioritized"]:
            return
        torch = self.torch
        idx = torch.as_tensor(idx, dtype=torch.int64, device=self.dev).contiguous()
        td = torch.as_tensor(td_error, dtype=torch.float64, device=self.dev).contiguous()
        prio = td.abs() + 1e-4
        self._ordered(self.stepper.exp_update_priorities, idx, prio)  # (prio is freed when this returns)

    def memory_size(self):
        """Transitions the memory holds (aigar_exp_info: a host round trip)."""
        if self.memory is None:
            raise RuntimeError("AgarVecEnv was created without memory=")
        return int(self.stepper.exp_info()["size"])

    def reset(self, seed=None):
        """Field.reset + every bot's reset (lastMass = None, history grids cleared);
        with several arenas, the desynchronising warm-up (aigar.py:833-837)."""
        seed = self.seed if seed is None else int(seed)
        self.stepper.reset(seed)
        if self.continuous is not None:
            self._ou_ac.zero_()
        self.age[:] = 0
        self._resets = 0
        if self.desync:
            self._desynchronise(seed)
        if self._scored:  # the episodes are scored from here: not the warm-up
            self.stepper.score_reset()
            self._ret.zero_()
            self.last_score.fill_(float("nan"))
            self.last_return.fill_(float("nan"))
        return self.observe()

    def _desynchronise(self, seed):
        """Arena k plays k * int(R / N) ticks from a fresh world before the first
        decision (collector k + 1 of aigar.py:833-837): all arenas are stepped
        together for (N - 1) * int(R / N) ticks and arena k gets its fresh world when
        k * int(R / N) of them are left; then Model.resetBots for every arena."""
        per = self.reset_limit // self.A
        total = (self.A - 1) * per
        for t in range(total + 1):
            fresh = [a for a in range(self.A) if t > 0 and total - a * per == t]
            if fresh:
                self.stepper.reset_arenas(fresh, [seed + 104729 * (a + 1) for a in fresh])
            if t == total:
                break
            # NN players: random points in their view (an untrained network's moves);
            # Greedy / Random bots: their own device policies
            self.stepper.policy_random(0.0, 0.0, seed ^ 0x5DEECE66D)
            self._others_move_and_tick()
        # Model.resetBots: every bot of every arena (the world goes on).  Still the host
        # round trip: load_state also re-lays the pellet rows and restarts the arena's
        # control block and epochs, which no device call does for a running world
        for a in range(self.A):
            self.stepper.load_state(self.stepper.get_state(a), a)
        self.age[:] = np.arange(self.A) * per

    def episode_over(self):
        """Arenas whose episode is over: the collector's test step > RESET_LIMIT -
        FRAME_SKIP_RATE + 2 (aigar.py:876)."""
        return self.age > self.reset_limit - self.skip + 2

    def observe(self):
        """A fresh tensor: the device buffer is rewritten by the next decision, so
        (s, a, r, s') tuples must not alias it (self.obs is that buffer)."""
        self._observe(self._nn_u8 if self._mixed else None)
        return self.obs.clone()

    def _observe(self, mask):
        self._obs_ready = True
        if self.pixels is not None:
            self.stepper.observe_pixel_state(self.obs, mask=mask)
        else:
            self.stepper.observe(self.obs, mask=mask)

    def _episode_ends(self):
        """Reset the arenas that reached RESET_LIMIT; returns the per-player done mask."""
        torch = self.torch
        done = torch.zeros(self.NP, dtype=torch.bool, device=self.dev)
        if self.reset_limit <= 0:
            return done
        self.age += self.skip + 1
        ended = np.nonzero(self.episode_over())[0]
        if not len(ended):
            return done
        mask = np.zeros(self.NP, np.uint8)
        seeds = []
        for a in ended:  # (ascending arena order)
            self._resets += 1
            seeds.append(self.seed + 7919 * self._resets)
            self.age[a] = 0
            mask[a * self.B:(a + 1) * self.B] = 1
        ended_t = torch.as_tensor(mask.astype(bool), device=self.dev)
        if self._scored:  # the finished episodes' rows, before the reset clears them (no host sync)
            self._read_score()
            self.last_score = torch.where(ended_t[:, None], self._score, self.last_score)
            self.last_return = torch.where(ended_t & self.nn, self._ret, self.last_return)
            self._ret = torch.where(ended_t, torch.zeros_like(self._ret), self._ret)
        self.stepper.reset_arenas(ended, seeds)  # one call, on the device
        if self.continuous is not None:  # (step_ac_calls' twin of the handle's Orn-Uhl state restarts too)
            self._ou_ac = torch.where(ended_t[:, None], torch.zeros_like(self._ou_ac), self._ou_ac)
        done[ended_t] = True
        # the new episodes' first states (NN players of the reset arenas)
        nn_reset = (mask & (self.roles == _abi.ROLE_NN)).astype(np.uint8)
        self._mask.copy_(torch.as_tensor(nn_reset))
        self._observe(self._mask)
        return done

    def step(self, actions):
        """actions: [n_players, 2..4] tensor/array in [0, 1] (rows of non-NN players are
        ignored) -> (obs, reward, alive, done).  The decision (skip + 1 ticks, every
        bot's moves, rewards, NN observations) is one graph replay."""
        torch = self.torch
        act = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions), device=self.dev)
        n = int(act.shape[1])
        buf = self._act.get(n)
        if buf is None:
            buf = self._act[n] = torch.empty((self.NP, n), dtype=torch.float64, device=self.dev)
        buf.copy_(act)
        self.stepper.env_step(buf, self._r, self.obs, self.enable_split, self.skip, self.reward_params)
        return self._after_decision()

    def _after_decision(self):
        torch = self.torch
        reward = self._r.clone()
        if self._scored:
            self._ret += torch.where(self.nn, reward, torch.zeros_like(reward))
        done = self._episode_ends()
        self._obs_ready = True
        alive = ~torch.isnan(self.obs.view(self.NP, -1)[:, 0]) & self.nn
        return self.obs.clone(), reward, alive, done

    def _read_score(self):
        self._ordered(self.stepper.score, self._score)

    def score(self):
        """[NP, 4] device tensor of the running episodes: samples, sum, max, deaths of
        every bot's mass list (Bot.getMassOverTime, bot.py:639-640)."""
        if not self._scored:
            raise RuntimeError("AgarVecEnv was created without score=True")
        self._read_score()
        return self._score.clone()

    def test_score(self, arena_mask=None):
        """(meanMass[A], maxMass[A]) of every arena's last finished episode, as
        performAgarioTest computes them (aigar.py:533-535): the mean over the arena's bots of
        their mean mass over time, and the largest mass any of them had.  NaN for an arena
        without a finished episode and where arena_mask (bool [A]) is False."""
        if not self._scored:
            raise RuntimeError("AgarVecEnv was created without score=True")
        torch = self.torch
        s = self.last_score.view(self.A, self.B, 4)
        mean = (s[:, :, 1] / s[:, :, 0]).mean(dim=1)
        top = s[:, :, 2].max(dim=1).values
        if arena_mask is not None:
            m = arena_mask if isinstance(arena_mask, torch.Tensor) else torch.as_tensor(np.asarray(arena_mask, bool))
            m = m.to(device=self.dev, dtype=torch.bool)
            nan = torch.full_like(mean, float("nan"))
            mean, top = torch.where(m, mean, nan), torch.where(m, top, nan)
        return mean, top

    def step_calls(self, actions):
        """The same decision as separate calls (apply_actions / Greedy bots / Random
        bots / step / rewards / observe); without the episode bookkeeping."""
        torch = self.torch
        act = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions), device=self.dev)
        act = act.to(device=self.dev, dtype=torch.float64).contiguous()
        reward = torch.zeros(self.NP, dtype=torch.float64, device=self.dev)
        for k in range(self.skip + 1):
            if k > 0:  # updateRewards on the skipped frames (bot.py:166-168)
                reward += self._reward_term(update_last=False)
            self.stepper.apply_actions(act, self.enable_split, skipping=k > 0, record=k == 0)
            self._others_move_and_tick()
        reward += self._reward_term(update_last=True)
        obs = self.observe()
        alive = ~torch.isnan(obs.view(self.NP, -1)[:, 0]) & self.nn
        return obs, reward, alive

    def _others_move_and_tick(self):
        """The Greedy and the Random bots' own device policies, then one tick."""
        if self._has_greedy:
            self.stepper.policy_greedy(self._greedy_split, self._greedy)
        if self._has_random:
            self.stepper.policy_random_bots()
        self.stepper.step(1)

    def _reward_term(self, update_last):
        """What updateRewards adds for every player (bot.py:167): getReward() while the bot
        has a lastMass, else 0 -- also with MASS_AS_REWARD, where getReward itself ignores
        lastMass; who has none shows as NaN in the mass-difference reward."""
        torch = self.torch
        prm = self.reward_params
        known = None
        if prm.mass_as_reward:
            plain = _abi.RewardParams(0, 0, prm.reward_term, prm.death_term, prm.death_factor, prm.reward_scale)
            self.stepper.rewards(plain, update_last=False, out=self._r)
            known = ~torch.isnan(self._r)
        self.stepper.rewards(prm, update_last=update_last, out=self._r)
        r = torch.nan_to_num(self._r)
        return r if known is None else torch.where(known, r, torch.zeros_like(r))

    def close(self):
        self.stepper.close()


class AgarSpgEnv(AgarVecEnv):
    """AgarVecEnv with the SPG learner's trainer: the keyword `search=` (True, or a
    dict that overrides samples, moving, replace, prio_evals, fused, noise, noise_decay, seed)
    beside `train="dpg"` or `train=dict(algorithm="dpg", ...)` selects the SPG step on the DPG
    trainer's critic: DPG's critic half, then every row's search among the stored action, the
    action a former search left in the memory's fifth field, the actor's action and `samples`
    Gaussian candidates, then the actor's regression towards the winners.  `train(n, u, zu)` makes n
    steps, one graph replay each; `search_noise` is the device double of the search's std (write
    it to follow a schedule of your own; the device multiplies it by noise_decay after every
    applied step).  `env.spg` is True and `env.dpg` False; the raw action is not stored
    (store_raw is off); `train_info()`, `train_td()`, `q_value()`, `get_weights(target=)` and the
    critic's accessors work as under DPG.  `search=True` reads OCACLA_EXPL_SAMPLES,
    OCACLA_MOVING_GAUSSIAN, OCACLA_REPLACE_TRANSITIONS, OCACLA_NOISE and OCACLA_NOISE_DECAY and
    DPG's names for the critic half; what the device does not do is refused by name
    (aigar_amd.net.spg_params).  With `search=None` this is AgarVecEnv.  The keyword lives here
    because AgarVecEnv's own signature is part of the facade's recorded surface."""

    def __init__(self, n_players, parameters=None, *, search=None, **options):
        self._search = search  # (read through _search_option while AgarVecEnv sets the noise and the trainer up)
        AgarVecEnv.__init__(self, n_players, parameters, **options)
        self._noise = None

    def _search_option(self):
        return self._search

    def train(self, n=1, u=None, zu=None):
        """n training steps.  u as AgarVecEnv.train's; zu: None (the search's own Philox draws) or
        the search's uniforms [n, batch, samples, 2, 16, 2] in [0, 1) (only with search=)."""
        if not self.spg:
            if zu is not None:
                raise ValueError("train: zu is the SPG search's (search=)")
            return AgarVecEnv.train(self, n, u)
        torch = self.torch
        n = int(n)
        if n < 1:
            raise ValueError("train: n must be at least 1")
        b, k = self.training["batch"], self.training["samples"]
        if u is not None:
            u = torch.as_tensor(u, dtype=torch.float64, device=self.dev).reshape(n, b).contiguous()
        if zu is not None and k:
            zu = torch.as_tensor(zu, dtype=torch.float64, device=self.dev).reshape(n, b, k, 2, 16, 2).contiguous()
        self._ordered(self.stepper.spg_step, n, u, zu if k else None)  # (u and zu are freed when this returns)

    @property
    def search_noise(self):
        """The device double of the search noise's std as a one-element float64 tensor: no copy,
        so writing it takes effect at the next step."""
        if not self.spg:
            raise RuntimeError("AgarSpgEnv was created without search= (the SPG trainer)")
        if self._noise is None:
            self._noise = _device_double(self.torch, self.stepper.spg_noise_ptr(), self.dev)
        return self._noise


def _device_double(torch, address, dev):
    """A one-element float64 tensor over the device double at `address` (owned by the handle)."""
    class _Ptr:
        __cuda_array_interface__ = {"shape": (1,), "typestr": "<f8", "data": (int(address), False), "version": 2}
    return torch.as_tensor(_Ptr(), device=dev)
