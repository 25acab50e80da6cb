"""What ``lm/models/bailing_moe.py`` / ``switch_layers.py`` need beyond ``mlx_shim.py`` (left as it is), as the MLX definitions in numpy:
``gather_mm`` with ``rhs_indices``, ``topk``, ``unflatten``, ``flatten`` and ``stop_gradient``.  ``install(mx, nn)`` adds them to the stand-in's ``mlx.core``; ``nn.GELU`` also
accepts ``approx="precise"`` (the default argument of ``SwitchMLP``, built at import and never called on this path)."""
import numpy as np


def install(mx, nn):
    wrap = lambda a: mx.array(np.asarray(a))

    def gather_mm(a, b, lhs_indices=None, rhs_indices=None, sorted_indices=False, stream=None):
        a, b = np.asarray(a), np.asarray(b)
        if lhs_indices is not None:
            a = a.reshape(-1, *a.shape[-2:])[np.asarray(lhs_indices).astype(np.int64)]
        if rhs_indices is not None:
            b = b.reshape(-1, *b.shape[-2:])[np.asarray(rhs_indices).astype(np.int64)]
        return wrap(np.matmul(a, b).astype(np.float32))

    def topk(a, k, axis=-1, stream=None):
        return wrap(np.take(np.sort(np.asarray(a), axis=axis), np.arange(-k, 0), axis=axis))

    def unflatten(a, axis, shape, stream=None):
        a = np.asarray(a)
        axis %= a.ndim
        return wrap(a.reshape(*a.shape[:axis], *shape, *a.shape[axis + 1:]))

    def flatten(a, start_axis=0, end_axis=-1, stream=None):
        a = np.asarray(a)
        s, e = start_axis % a.ndim, end_axis % a.ndim
        return wrap(a.reshape(*a.shape[:s], -1, *a.shape[e + 1:]))

    for f in (gather_mm, topk, unflatten, flatten):
        setattr(mx, f.__name__, f)
    mx.stop_gradient = lambda a, stream=None: a

    base = nn.GELU

    class GELU(base):
        def __init__(self, approx="none"):
            super().__init__("none" if approx == "precise" else approx)

    nn.GELU = GELU
