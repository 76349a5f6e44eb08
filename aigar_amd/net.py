"""The learners' acting network as the device runs it (include/aigar.h aigar_net*;
DESIGN.md §4j): the reference's parameters -> a network specification, and a trainer's
weights -> the Keras-layout float32 arrays the device takes.

The device evaluates MLPs only: up to five dense layers of at most 256 units, relu or
linear hidden layers, a linear (Q) or sigmoid (actor) head.  Everything else the reference
can build is refused here, at configuration, with a message that names the setting."""
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
