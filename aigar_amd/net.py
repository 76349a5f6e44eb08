"""The learners' acting network as the device runs it (include/aigar.h aigar_net*;
DESIGN.md §4j): the reference's parameters -> a network specification, and a trainer's
weights -> the Keras-layout float32 arrays the device takes.

The device evaluates MLPs: up to five dense layers of at most 256 units, relu or linear
hidden layers, a linear (Q) or sigmoid (actor) head; and, in front of one, the conv layers of
the reference's CNN over the pixel state (cnn_spec, cnn_weights_from_torch).
Everything else the reference can build is refused here, at configuration, with a message
that names the setting."""
import collections

import numpy as np

from . import _abi

NetSpec = collections.namedtuple("NetSpec", "n_in units hidden out")


def _get(parameters, name, default):
    if parameters is None:
        return default
    if isinstance(parameters, dict):
        return parameters.get(name, default)
    return getattr(parameters, name, default)


def mlp_spec(parameters=None, head="q", n_in=None, n_out=None):
    """NetSpec of the reference's acting network: head "q" reads Q_LAYERS,
    ACTIVATION_FUNC_HIDDEN and ACTIVATION_FUNC_OUTPUT (network.py:207-241), head "actor"
    CACLA_ACTOR_LAYERS (DPG_ACTOR_LAYERS when ALGORITHM is "DPG") and
    ACTIVATION_FUNC_HIDDEN_POLICY with a sigmoid head (actorCritic.py:219-330).  Hidden
    layers of 0 units are skipped, as the reference skips them.  n_in is the state length
    and n_out the head's width (the number of discrete actions / of action values); None
    leaves them to the caller (AgarVecEnv fills them in)."""
    if head not in _abi.NET_HEADS:
        raise ValueError("mlp_spec: head must be one of %s" % sorted(_abi.NET_HEADS))
    g = lambda n, d: _get(parameters, n, d)
    if g("NEURON_TYPE", "MLP") != "MLP":
        raise ValueError("mlp_spec: NEURON_TYPE = %r: the device network is an MLP" % (g("NEURON_TYPE", "MLP"),))
    if g("CNN_REPR", False):
        raise ValueError("mlp_spec: CNN_REPR: the device network takes no CNN / pixel state")
    if g("USE_ACTION_AS_INPUT", False):
        raise ValueError("mlp_spec: USE_ACTION_AS_INPUT is not supported by the device network")
    if head == "q":
        layers, hidden = g("Q_LAYERS", (100, 100)), g("ACTIVATION_FUNC_HIDDEN", "relu")
        out = g("ACTIVATION_FUNC_OUTPUT", "linear")
    else:
        key = "DPG_ACTOR_LAYERS" if g("ALGORITHM", "CACLA") == "DPG" else "CACLA_ACTOR_LAYERS"
        layers, hidden = g(key, (100, 100)), g("ACTIVATION_FUNC_HIDDEN_POLICY", "relu")
        out = "sigmoid"
    if g("BATCHNORM", False):
        raise ValueError("mlp_spec: BATCHNORM is not supported by the device network")
    if hidden not in ("relu", "linear"):
        raise ValueError("mlp_spec: hidden activation %r is not supported by the device network (relu, linear)"
                         % (hidden,))
    if out not in ("linear", "sigmoid"):
        raise ValueError("mlp_spec: output activation %r is not supported by the device network (linear, sigmoid)"
                         % (out,))
    units = tuple(int(v) for v in layers if int(v) > 0)
    if len(units) + 1 > _abi.NET_MAX_LAYERS:
        raise ValueError("mlp_spec: %d hidden layers, at most %d" % (len(units), _abi.NET_MAX_LAYERS - 1))
    if n_out is not None:
        units = units + (int(n_out),)
    if any(v > _abi.NET_MAX_UNITS for v in units):
        raise ValueError("mlp_spec: a layer of %d units, at most %d" % (max(units), _abi.NET_MAX_UNITS))
    if n_in is not None and not 1 <= int(n_in) <= _abi.NET_MAX_IN:
        raise ValueError("mlp_spec: %d inputs, at most %d" % (n_in, _abi.NET_MAX_IN))
    return NetSpec(None if n_in is None else int(n_in), units, hidden, out)


CnnSpec = collections.namedtuple("CnnSpec", "side channels convs n_flat units hidden out")


class _Dense:
    """The parameters as mlp_spec reads them for the dense layers behind the conv part."""

    def __init__(self, parameters):
        self._p = parameters

    def __getattr__(self, name):
        if name == "CNN_REPR":
            return False
        if name.startswith("_"):
            raise AttributeError(name)
        v = _get(self._p, name, _Dense)
        if v is _Dense:
            raise AttributeError(name)
        return v


def conv_out_side(side, convs):
    """The output side of every conv layer: (in - k) // s + 1 (valid padding)."""
    out = []
    for k, s, _ in convs:
        side = (side - k) // s + 1
        out.append(side)
    return out


def cnn_spec(parameters=None, head="q", n_out=None):
    """CnnSpec of the reference's CNN over the pixel state (CNN_REPR with CNN_P_REPR;
    network.py:154-183, actorCritic.py:122-136): the conv layers CNN_L1/2/3 = (kernel, stride,
    filters) that CNN_USE_L1/2/3 switch on, the image side CNN_INPUT_DIM_* of the first of them
    (rgbGenerator.py:16-21), 1 channel (3 with CNN_P_RGB), doubled by CNN_LAST_GRID; then the
    dense layers and activations mlp_spec reads for the head, on the flattened length n_flat.
    n_out as in mlp_spec."""
    g = lambda n, d: _get(parameters, n, d)
    if g("CNN_REPR", False) and not g("CNN_P_REPR", False):
        raise ValueError("cnn_spec: CNN_REPR without CNN_P_REPR (the CNN over the grid view) is not supported by the "
                         "device network")
    if g("CNN_P_INCEPTION", False):
        raise ValueError("cnn_spec: CNN_P_INCEPTION is not supported by the device network")
    use = [bool(g("CNN_USE_L1", True)), bool(g("CNN_USE_L2", True)), bool(g("CNN_USE_L3", False))]
    layers = [g("CNN_L1", (8, 4, 32)), g("CNN_L2", (4, 2, 64)), g("CNN_L3", (3, 1, 64))]
    dims = [g("CNN_INPUT_DIM_1", 42), g("CNN_INPUT_DIM_2", 84), g("CNN_INPUT_DIM_3", 42)]
    if not any(use):
        raise ValueError("cnn_spec: none of CNN_USE_L1, CNN_USE_L2, CNN_USE_L3 is set: no conv layer")
    side = int(dims[use.index(True)])
    channels = (3 if g("CNN_P_RGB", False) else 1) * (2 if g("CNN_LAST_GRID", False) else 1)
    if not 1 <= side <= _abi.CONV_MAX_SIDE:
        raise ValueError("cnn_spec: CNN_INPUT_DIM_%d = %d is outside 1..%d" % (use.index(True) + 1, side,
                                                                               _abi.CONV_MAX_SIDE))
    convs, cur = [], side
    for i in range(3):
        if not use[i]:
            continue
        name = "CNN_L%d" % (i + 1)
        if len(layers[i]) != 3:
            raise ValueError("cnn_spec: %s must be (kernel, stride, filters), got %r" % (name, layers[i]))
        k, s, f = (int(v) for v in layers[i])
        if not 1 <= k <= _abi.CONV_MAX_KERNEL or not 1 <= s <= _abi.CONV_MAX_KERNEL:
            raise ValueError("cnn_spec: %s = %r: kernel and stride must be in 1..%d" % (name, tuple(layers[i]),
                                                                                      _abi.CONV_MAX_KERNEL))
        if not 1 <= f <= _abi.CONV_MAX_FILTERS:
            raise ValueError("cnn_spec: %s = %r: filters must be in 1..%d" % (name, tuple(layers[i]),
                                                                             _abi.CONV_MAX_FILTERS))
        if cur < k:
            raise ValueError("cnn_spec: %s = %r has no output on an input of side %d" % (name, tuple(layers[i]), cur))
        cur = (cur - k) // s + 1
        convs.append((k, s, f))
    n_flat = cur * cur * convs[-1][2]
    if n_flat > _abi.NET_MAX_IN:
        raise ValueError("cnn_spec: the flattened length %d (%d x %d x %d) is above %d: CNN_USE_L*"
                         % (n_flat, cur, cur, convs[-1][2], _abi.NET_MAX_IN))
    try:
        dense = mlp_spec(_Dense(parameters), head, n_in=n_flat, n_out=n_out)
    except ValueError as e:
        raise ValueError(str(e).replace("mlp_spec:", "cnn_spec:", 1)) from None
    return CnnSpec(side, channels, tuple(convs), n_flat, dense.units, dense.hidden, dense.out)


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def cnn_weights_from_torch(source, spec):
    """[(W [k, k, Cin, F], b [F]), ..., (W [in, out], b [out]), ...] float32 numpy arrays in
    Keras' layout for a CnnSpec, the conv pairs first: from a torch module or state dict of
    nn.Conv2d layers (weight [out, in, kh, kw] -> [kh, kw, in, out]) followed by nn.Linear
    layers (weight [out, in], transposed; the first one's input, which a torch Flatten of NCHW
    gives in (c, y, x) order, is permuted to the device's (y, x, c) order), or from a plain
    list of Keras-layout arrays, flat or in pairs, which is passed through."""
    if hasattr(source, "state_dict"):
        source = source.state_dict()
    out = []
    if isinstance(source, dict):
        first = True
        for k, w in source.items():
            if not k.endswith("weight") or getattr(w, "ndim", 0) not in (2, 4):
                continue
            w = _np(w)
            b = source.get(k[:-len("weight")] + "bias")
            b = np.zeros(w.shape[0], np.float32) if b is None else _np(b)
            if w.ndim == 4:
                w = w.transpose(2, 3, 1, 0)
            else:
                w = w.T
                if first:
                    f = spec.convs[-1][2]
                    o = conv_out_side(spec.side, spec.convs)[-1]
                    if w.shape[0] != f * o * o:
                        raise ValueError("cnn_weights_from_torch: the first Linear has %d inputs, the conv part gives "
                                         "%d" % (w.shape[0], f * o * o))
                    w = w.reshape(f, o, o, w.shape[1]).transpose(1, 2, 0, 3).reshape(f * o * o, w.shape[1])
                    first = False
            out.append((np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)))
    else:
        items = list(source)
        if items and isinstance(items[0], (tuple, list)) and len(items[0]) == 2:
            pairs = items
        else:
            if len(items) % 2:
                raise ValueError("cnn_weights_from_torch: a flat list must be [W0, b0, W1, b1, ...]")
            pairs = list(zip(items[0::2], items[1::2]))
        out = [(np.ascontiguousarray(_np(w), np.float32), np.ascontiguousarray(_np(b), np.float32)) for w, b in pairs]
    shapes, cin = [], spec.channels
    for k, _, f in spec.convs:
        shapes.append((k, k, cin, f))
        cin = f
    n = spec.n_flat
    for u in spec.units:
        shapes.append((n, u))
        n = u
    got = [w.shape for w, _ in out]
    if got != shapes or any(b.shape != (w.shape[-1],) for w, b in out):
        raise ValueError("cnn_weights_from_torch: expected kernels of shapes %s with their biases, got %s" % (shapes, got))
    return out


def weights_from_torch(source):
    """[(W [in, out], b [out]), ...] float32 numpy arrays in Keras' layout from a torch
    module or state dict of nn.Linear layers (whose weight is [out, in]: transposed here; the
    layers in the dict's order), or from a plain list of Keras-layout arrays [W0, b0, W1, b1,
    ...] or [(W0, b0), ...], which is passed through."""
    if hasattr(source, "state_dict"):
        source = source.state_dict()
    if isinstance(source, dict):
        ws = [(k, v) for k, v in source.items() if k.endswith("weight") and getattr(v, "ndim", 0) == 2]
        out = []
        for k, w in ws:
            b = source.get(k[:-len("weight")] + "bias")
            w = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
            if b is None:
                b = np.zeros(w.shape[0], np.float32)
            b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
            out.append((np.ascontiguousarray(w.T, np.float32), np.ascontiguousarray(b, np.float32)))
        if not out:
            raise ValueError("weights_from_torch: no 2-d '...weight' entries")
        return out
    items = list(source)
    if items and isinstance(items[0], (tuple, list)) and len(items[0]) == 2 and np.ndim(items[0][0]) == 2:
        pairs = items
    else:
        if len(items) % 2:
            raise ValueError("weights_from_torch: a flat list must be [W0, b0, W1, b1, ...]")
        pairs = list(zip(items[0::2], items[1::2]))
    out = []
    for w, b in pairs:
        w = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
        b = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
        if w.ndim != 2 or b.shape != (w.shape[1],):
            raise ValueError("weights_from_torch: expected W [in, out] and b [out], got %s and %s" % (w.shape, b.shape))
        out.append((np.ascontiguousarray(w, np.float32), np.ascontiguousarray(b, np.float32)))
    return out


def weights_to_torch(weights, module):
    """The inverse of weights_from_torch: [(W [in, out], b [out]), ...] (numpy arrays or
    tensors, Keras' layout) into the nn.Linear layers of a torch module, in order (weight
    [out, in] = W transposed).  Returns the module."""
    import torch
    layers = [m for m in module.modules() if isinstance(m, torch.nn.Linear)]
    if len(layers) != len(weights):
        raise ValueError("weights_to_torch: %d layers given, the module has %d nn.Linear" % (len(weights), len(layers)))
    with torch.no_grad():
        for m, (W, b) in zip(layers, weights):
            W, b = torch.as_tensor(_np(W)), torch.as_tensor(_np(b))
            if tuple(W.shape) != (m.in_features, m.out_features):
                raise ValueError("weights_to_torch: W is %s, the layer takes (%d, %d)"
                                 % (tuple(W.shape), m.in_features, m.out_features))
            m.weight.copy_(W.t().to(m.weight))
            if m.bias is not None:
                m.bias.copy_(b.to(m.bias))
    return module


def cnn_weights_to_torch(pairs, spec, module=None):
    """The inverse of cnn_weights_from_torch: the conv pairs (W [k, k, Cin, F], b [F]) first, then
    the dense pairs (W [in, out], b [out]), numpy arrays or tensors in Keras' layout, for a
    CnnSpec -> an ordered state dict {"conv0.weight": [F, Cin, k, k], "conv0.bias", ...,
    "fc0.weight": [out, in], "fc0.bias", ...} of float32 tensors, the first Linear's input
    permuted from the device's (y, x, c) order back to the (c, y, x) order of a torch Flatten of
    NCHW.  With a module, its nn.Conv2d and nn.Linear layers, in order, are loaded instead and
    the module is returned."""
    import collections
    import torch
    pairs = [(np.asarray(_np(W), np.float32), np.asarray(_np(b), np.float32)) for W, b in pairs]
    nc = len(spec.convs)
    if len(pairs) != nc + len(spec.units):
        raise ValueError("cnn_weights_to_torch: %d pairs given, the spec has %d conv and %d dense layers"
                         % (len(pairs), nc, len(spec.units)))
    cnn_weights_from_torch(pairs, spec)  # (the shapes)
    out = collections.OrderedDict()
    for l, (W, b) in enumerate(pairs):
        if l < nc:
            w, name = W.transpose(3, 2, 0, 1), "conv%d" % l
        else:
            if l == nc:
                f = spec.convs[-1][2]
                o = conv_out_side(spec.side, spec.convs)[-1]
                W = W.reshape(o, o, f, W.shape[1]).transpose(2, 0, 1, 3).reshape(f * o * o, W.shape[1])
            w, name = W.T, "fc%d" % (l - nc)
        out[name + ".weight"] = torch.as_tensor(np.ascontiguousarray(w))
        out[name + ".bias"] = torch.as_tensor(np.ascontiguousarray(b))
    if module is None:
        return out
    layers = [m for m in module.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]
    if len(layers) != len(pairs):
        raise ValueError("cnn_weights_to_torch: %d pairs given, the module has %d nn.Conv2d / nn.Linear"
                         % (len(pairs), len(layers)))
    with torch.no_grad():
        for m, name in zip(layers, list(out)[0::2]):
            w, b = out[name], out[name[:-len("weight")] + "bias"]
            if tuple(w.shape) != tuple(m.weight.shape):
                raise ValueError("cnn_weights_to_torch: %s is %s, the layer's weight %s"
                                 % (name, tuple(w.shape), tuple(m.weight.shape)))
            m.weight.copy_(w.to(m.weight))
            if m.bias is not None:
                m.bias.copy_(b.to(m.bias))
    return module


def train_params(parameters=None):
    """The device trainer's settings from the reference's parameters: Q-learning
    with Keras' Adam, what qLearning.py and network.py do by default.  Everything else the
    reference can train with is refused here, by the name of the setting."""
    g = lambda n, d: _get(parameters, n, d)
    if g("OPTIMIZER", "Adam") != "Adam":
        raise ValueError("train: OPTIMIZER = %r: the device trainer is Adam" % (g("OPTIMIZER", "Adam"),))
    for name in ("AMSGRAD", "GRADIENT_CLIP", "GRADIENT_CLIP_NORM", "Q_WEIGHT_DECAY", "DROPOUT", "ENABLE_QV",
                 "USE_ACTION_AS_INPUT", "END_DISCOUNT", "CNN_REPR", "BATCHNORM"):
        if g(name, 0):
            raise ValueError("train: %s = %r is not supported by the device trainer" % (name, g(name, 0)))
    if g("NEURON_TYPE", "MLP") != "MLP":
        raise ValueError("train: NEURON_TYPE = %r: the device trainer takes no LSTM" % (g("NEURON_TYPE", "MLP"),))
    if g("TD", 0) != 0:
        raise ValueError("train: TD = %r: only one-step targets (TD = 0)" % (g("TD", 0),))
    return {"batch": int(g("MEMORY_BATCH_LEN", 32)), "min_size": int(g("NUM_EXPS_BEFORE_TRAIN", 32)),
            "target_steps": int(g("TARGET_NETWORK_STEPS", 1500)), "lr": float(g("ALPHA", 0.001)), "beta1": 0.9,
            "beta2": 0.999, "epsilon": 1e-7, "discount": float(g("DISCOUNT", 0.9))}


def critic_spec(parameters=None, n_in=None):
    """NetSpec of the CACLA learner's critic V(s) (actorCritic.py ValueNetwork): CACLA_CRITIC_LAYERS
    hidden layers with ACTIVATION_FUNC_HIDDEN and one linear output.  n_in as in mlp_spec."""
    g = lambda n, d: _get(parameters, n, d)
    hidden = g("ACTIVATION_FUNC_HIDDEN", "relu")
    if hidden not in ("relu", "linear"):
        raise ValueError("critic_spec: hidden activation %r is not supported by the device network (relu, linear)"
                         % (hidden,))
    units = tuple(int(v) for v in g("CACLA_CRITIC_LAYERS", (100, 100)) if int(v) > 0)
    if len(units) + 1 > _abi.NET_MAX_LAYERS:
        raise ValueError("critic_spec: %d hidden layers, at most %d" % (len(units), _abi.NET_MAX_LAYERS - 1))
    if any(v > _abi.NET_MAX_UNITS for v in units):
        raise ValueError("critic_spec: a layer of %d units, at most %d" % (max(units), _abi.NET_MAX_UNITS))
    if n_in is not None and not 1 <= int(n_in) <= _abi.NET_MAX_IN:
        raise ValueError("critic_spec: %d inputs, at most %d" % (n_in, _abi.NET_MAX_IN))
    return NetSpec(None if n_in is None else int(n_in), units + (1,), hidden, "linear")


def actrain_params(parameters=None):
    """The device's CACLA trainer's settings from the reference's parameters: what
    actorCritic.py does for ALGORITHM == "CACLA" by default, CACLA-Var included (var_epochs is the
    device's cap on a row's actor epochs, 8, when CACLA_VAR_ENABLED; 0: plain CACLA).  Everything
    else the reference can train an actor-critic learner with is refused here, by the name of the
    setting."""
    g = lambda n, d: _get(parameters, n, d)
    if g("ALGORITHM", "CACLA") != "CACLA":
        raise ValueError("actrain: ALGORITHM = %r: the device's actor-critic trainer is CACLA (for DPG pass train='dpg')"
                         % (g("ALGORITHM", "CACLA"),))
    for name in ("OPTIMIZER", "OPTIMIZER_POLICY"):
        if g(name, "Adam") != "Adam":
            raise ValueError("actrain: %s = %r: the device trainer is Adam" % (name, g(name, "Adam")))
    for name in ("OCACLA_ENABLED", "CACLA_UPDATE_ON_NEGATIVE_TD", "CACLA_CRITIC_WEIGHT_DECAY", "CACLA_OFF_POLICY_CORR",
                 "ACTOR_IS", "AC_ACTOR_TDE", "AC_DELAY_ACTOR_TRAINING", "AC_ACTOR_TRAINING_START", "AMSGRAD",
                 "END_DISCOUNT", "DROPOUT", "GRADIENT_CLIP", "GRADIENT_CLIP_NORM", "USE_ACTION_AS_INPUT", "CNN_REPR",
                 "BATCHNORM"):
        if g(name, 0):
            raise ValueError("actrain: %s = %r is not supported by the device trainer" % (name, g(name, 0)))
    if g("NEURON_TYPE", "MLP") != "MLP":
        raise ValueError("actrain: NEURON_TYPE = %r: the device trainer takes no LSTM" % (g("NEURON_TYPE", "MLP"),))
    if g("TD", 0) != 0:
        raise ValueError("actrain: TD = %r: only one-step targets (TD = 0)" % (g("TD", 0),))
    return {"batch": int(g("MEMORY_BATCH_LEN", 32)), "min_size": int(g("NUM_EXPS_BEFORE_TRAIN", 32)),
            "target_steps": int(g("TARGET_NETWORK_STEPS", 1500)),
            "var_epochs": _abi.ACTRAIN_MAX_EPOCHS if g("CACLA_VAR_ENABLED", True) else 0,
            "critic_lr": float(g("CACLA_CRITIC_ALPHA", 0.000075)), "actor_lr": float(g("CACLA_ACTOR_ALPHA", 0.0005)),
            "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-7, "discount": float(g("DISCOUNT", 0.9)),
            "var_start": float(g("CACLA_VAR_START", 1)), "var_beta": float(g("CACLA_VAR_BETA", 0.001))}


def qcritic_spec(parameters=None, n_in=None, n_act=None):
    """NetSpec of the DPG learner's critic Q(s, a) (actorCritic.py ActionValueNetwork with
    DPG_FEED_ACTION_IN_LAYER = 1): the input row is the state, then the action, so its n_in is
    n_in + n_act (None while either is); DPG_CRITIC_LAYERS hidden layers with DPG_CRITIC_FUNC and
    one linear output."""
    g = lambda n, d: _get(parameters, n, d)
    hidden = g("DPG_CRITIC_FUNC", "relu")
    if hidden not in ("relu", "linear"):
        raise ValueError("qcritic_spec: DPG_CRITIC_FUNC = %r is not supported by the device network (relu, linear)"
                         % (hidden,))
    units = tuple(int(v) for v in g("DPG_CRITIC_LAYERS", (100, 100)) if int(v) > 0)
    if len(units) + 1 > _abi.NET_MAX_LAYERS:
        raise ValueError("qcritic_spec: %d hidden layers, at most %d" % (len(units), _abi.NET_MAX_LAYERS - 1))
    if any(v > _abi.NET_MAX_UNITS for v in units):
        raise ValueError("qcritic_spec: a layer of %d units, at most %d" % (max(units), _abi.NET_MAX_UNITS))
    if n_act is not None and not 1 <= int(n_act) <= 4:
        raise ValueError("qcritic_spec: %d actions, 1..4" % (n_act,))
    n = None if n_in is None or n_act is None else int(n_in) + int(n_act)
    if n is not None and not 1 <= n <= _abi.NET_MAX_IN:
        raise ValueError("qcritic_spec: %d inputs, at most %d" % (n, _abi.NET_MAX_IN))
    return NetSpec(n, units + (1,), hidden, "linear")


def dpg_params(parameters=None):
    """The device's DPG trainer's settings from the reference's parameters: what
    actorCritic.py does for ALGORITHM == "DPG" by default (an absent ALGORITHM counts as "DPG"
    here).  SOFT_TARGET_UPDATES picks tau = DPG_TAU; without it tau = 0 and both targets are copied
    every TARGET_NETWORK_STEPS.  Everything else the reference can train a DPG learner with is
    refused here, by the name of the setting."""
    g = lambda n, d: _get(parameters, n, d)
    if g("ALGORITHM", "DPG") != "DPG":
        raise ValueError("dpg: ALGORITHM = %r: this is the device's DPG trainer" % (g("ALGORITHM", "DPG"),))
    for name in ("OPTIMIZER", "OPTIMIZER_POLICY", "DPG_ACTOR_OPTIMIZER"):
        if g(name, "Adam") != "Adam":
            raise ValueError("dpg: %s = %r: the device trainer is Adam" % (name, g(name, "Adam")))
    for name in ("OCACLA_ENABLED", "CACLA_UPDATE_ON_NEGATIVE_TD", "CACLA_CRITIC_WEIGHT_DECAY", "CACLA_OFF_POLICY_CORR",
                 "ACTOR_IS", "AC_ACTOR_TDE", "AC_DELAY_ACTOR_TRAINING", "AC_ACTOR_TRAINING_START", "AMSGRAD",
                 "END_DISCOUNT", "DROPOUT", "GRADIENT_CLIP", "GRADIENT_CLIP_NORM", "USE_ACTION_AS_INPUT", "CNN_REPR",
                 "BATCHNORM", "DPG_USE_CACLA", "DPG_CACLA_ALTERNATION", "DPG_CACLA_INV_ALTERNATION",
                 "DPG_CRITIC_WEIGHT_DECAY", "DPG_ACTOR_NESTEROV"):
        if g(name, 0):
            raise ValueError("dpg: %s = %r is not supported by the device trainer" % (name, g(name, 0)))
    if g("DPG_FEED_ACTION_IN_LAYER", 1) != 1:
        raise ValueError("dpg: DPG_FEED_ACTION_IN_LAYER = %r: the action enters the critic beside the state (1)"
                         % (g("DPG_FEED_ACTION_IN_LAYER", 1),))
    for name in ("DPG_USE_TARGET_MODELS", "DPG_USE_DPG_ACTOR_TRAINING"):
        if not g(name, True):
            raise ValueError("dpg: %s = %r: the device trainer always does" % (name, g(name, True)))
    if g("NEURON_TYPE", "MLP") != "MLP":
        raise ValueError("dpg: NEURON_TYPE = %r: the device trainer takes no LSTM" % (g("NEURON_TYPE", "MLP"),))
    if g("TD", 0) != 0:
        raise ValueError("dpg: TD = %r: only one-step targets (TD = 0)" % (g("TD", 0),))
    soft = bool(g("SOFT_TARGET_UPDATES", True))
    return {"batch": int(g("MEMORY_BATCH_LEN", 32)), "min_size": int(g("NUM_EXPS_BEFORE_TRAIN", 32)),
            "target_steps": int(g("TARGET_NETWORK_STEPS", 1500)),
            "critic_lr": float(g("DPG_CRITIC_ALPHA", 0.0005)), "actor_lr": float(g("DPG_ACTOR_ALPHA", 0.0001)),
            "beta1": 0.9, "beta2": 0.999, "epsilon": 1e-7, "discount": float(g("DISCOUNT", 0.9)),
            "tau": float(g("DPG_TAU", 0.001)) if soft else 0.0, "q_increase": float(g("DPG_Q_VAL_INCREASE", 2))}


def spg_params(parameters=None):
    """The device's SPG trainer's settings from the reference's parameters: what
    actorCritic.py does for OCACLA_ENABLED (ALGORITHM "SPG"; an absent ALGORITHM counts as "SPG"
    here): the critic half under DPG's names, the search under OCACLA_EXPL_SAMPLES,
    OCACLA_MOVING_GAUSSIAN, OCACLA_REPLACE_TRANSITIONS, OCACLA_NOISE and OCACLA_NOISE_DECAY, and
    the memory's priority from Q(s, a) as the reference hands it over (prio_evals).  What
    dpg_params refuses is refused here too, except OCACLA_ENABLED; so are OCACLA_ONLINE_SAMPLES,
    Orn-Uhl search noise and CNN_REPR, each by its name."""
    g = lambda n, d: _get(parameters, n, d)
    if g("ALGORITHM", "SPG") != "SPG":
        raise ValueError("spg: ALGORITHM = %r: this is the device's SPG trainer" % (g("ALGORITHM", "SPG"),))
    if g("OCACLA_ONLINE_SAMPLES", 0):
        raise ValueError("spg: OCACLA_ONLINE_SAMPLES = %r: the decision samples no actions on the device"
                         % (g("OCACLA_ONLINE_SAMPLES", 0),))
    if g("NOISE_TYPE", "Gaussian") != "Gaussian":
        raise ValueError("spg: NOISE_TYPE = %r: the search's noise is Gaussian" % (g("NOISE_TYPE", "Gaussian"),))
    if g("CNN_REPR", False):
        raise ValueError("spg: CNN_REPR = %r: CNN critics are not trained on the device" % (g("CNN_REPR", False),))
    samples = int(g("OCACLA_EXPL_SAMPLES", 5))
    if not 0 <= samples <= _abi.SPG_MAX_SAMPLES:
        raise ValueError("spg: OCACLA_EXPL_SAMPLES = %d: 0..%d" % (samples, _abi.SPG_MAX_SAMPLES))
    as_dpg = {k: g(k, None) for k in _DPG_NAMES if g(k, None) is not None}
    as_dpg["ALGORITHM"] = "DPG"
    as_dpg["OCACLA_ENABLED"] = False
    try:
        p = dpg_params(as_dpg)
    except ValueError as e:
        raise ValueError("spg" + str(e)[3:]) from None
    del p["q_increase"]  # (the search has no Q-value increase)
    p.update(samples=samples, moving=bool(g("OCACLA_MOVING_GAUSSIAN", True)),
             replace=bool(g("OCACLA_REPLACE_TRANSITIONS", False)), prio_evals=True, fused=True,
             noise=float(g("OCACLA_NOISE", 1)), noise_decay=float(g("OCACLA_NOISE_DECAY", 0.0004 ** (1.0 / 500000))), seed=0)
    return p


# every setting dpg_params reads (spg_params hands them on)
_DPG_NAMES = ("OPTIMIZER", "OPTIMIZER_POLICY", "DPG_ACTOR_OPTIMIZER", "CACLA_UPDATE_ON_NEGATIVE_TD", "CACLA_CRITIC_WEIGHT_DECAY",
              "CACLA_OFF_POLICY_CORR", "ACTOR_IS", "AC_ACTOR_TDE", "AC_DELAY_ACTOR_TRAINING", "AC_ACTOR_TRAINING_START",
              "AMSGRAD", "END_DISCOUNT", "DROPOUT", "GRADIENT_CLIP", "GRADIENT_CLIP_NORM", "USE_ACTION_AS_INPUT", "BATCHNORM",
              "DPG_USE_CACLA", "DPG_CACLA_ALTERNATION", "DPG_CACLA_INV_ALTERNATION", "DPG_CRITIC_WEIGHT_DECAY",
              "DPG_ACTOR_NESTEROV", "DPG_FEED_ACTION_IN_LAYER", "DPG_USE_TARGET_MODELS", "DPG_USE_DPG_ACTOR_TRAINING",
              "NEURON_TYPE", "TD", "SOFT_TARGET_UPDATES", "MEMORY_BATCH_LEN", "NUM_EXPS_BEFORE_TRAIN", "TARGET_NETWORK_STEPS",
              "DPG_CRITIC_ALPHA", "DPG_ACTOR_ALPHA", "DISCOUNT", "DPG_TAU")
