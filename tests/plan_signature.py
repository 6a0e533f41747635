"""Host-only launch-list signature of a lowered plan (test helper).

A network is built with ``allocate=False`` and given CPU tensors and a stub library, so ``Network.plan`` and
``Lowering.build_backward`` run without a GPU.  Every launch becomes (name, library function, arguments), with each pointer
argument rewritten as (tensor role, byte offset) and every ConvDesc spelled out field by field.  Two revisions of the engine
that lower a network to the same signature issue the same kernels with the same arguments."""
import ctypes as C

import torch


class _StubLib:
    def __getattr__(self, name):
        def fn(*args):
            raise RuntimeError(f"stub {name} called")
        fn.__name__ = name
        return fn


def _stub_network(net):
    dev = torch.device("cpu")
    net.device = dev
    net.lib = _StubLib()
    net.P = torch.zeros(net.n_params)
    net.S_mean, net.S_var = torch.zeros(net.CB), torch.ones(net.CB)
    net.W_train = torch.zeros(net.n_kernel, dtype=net.train_dtype)
    net.Wt_train = torch.zeros(net.n_kernel, dtype=net.train_dtype)
    net.W_infer = torch.zeros(net.n_kernel, dtype=net.infer_dtype)
    net.fold_bias = torch.zeros(net.CB)
    net.table = torch.zeros(len(net.layers), 8, dtype=torch.int32)
    net.G = None
    net.alloc_grads()
    return net


def _tensors(net, plan):
    out = {}
    for k in ("P", "S_mean", "S_var", "W_train", "Wt_train", "W_infer", "fold_bias", "G", "Gacc", "table"):
        out["net." + k] = getattr(net, k)
    for k, v in vars(plan).items():
        if isinstance(v, torch.Tensor):
            out["plan." + k] = v
    for name, b in plan.bufs.items():
        for part in ("act", "raw", "grad"):
            t = getattr(b, part)
            if t is not None:
                out[f"buf.{name}.{part}"] = t
    for i, r in enumerate(plan.recs):
        for k, v in r.extra.items():
            if isinstance(v, torch.Tensor):
                out[f"rec{i}.{k}"] = v
    for k, v in getattr(plan, "_dup", {}).items():
        out["dup." + k] = v
    return out


def _canon(v, spans):
    if isinstance(v, C.Structure):
        return [(f, _canon(getattr(v, f), spans)) for f, _ in v._fields_]
    if isinstance(v, C.Array):
        return [_canon(e, spans) for e in v]
    if isinstance(v, C.c_void_p):
        v = v.value
    if isinstance(v, C._Pointer) or type(v).__name__ == "CArgObject":
        v = C.cast(v._obj if hasattr(v, "_obj") else v, C.c_void_p).value
    if isinstance(v, int) and v > (1 << 20):
        for name, lo, hi in spans:
            if lo <= v <= hi:
                return ("ptr", name, v - lo)
        return ("ptr", "?")
    if isinstance(v, float):
        return round(v, 9)
    return v


def signature(net, N, training, loss="triplet"):
    """[(op name, function name, canonical arguments)] of the forward (and, for training plans, backward) launch list."""
    _stub_network(net)
    plan = net.plan(N, training=training, loss=loss if training else None)
    if training:
        plan.build_backward(torch.zeros(N, net.E))
    spans = sorted(((n, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for n, t in _tensors(net, plan).items()
                    if t.numel() > 0), key=lambda s: (s[1], s[0]))
    ops = plan.fwd + (plan.bwd if training else [])
    out = []
    for op in ops:
        args = []
        for a in op.args:
            if type(a).__name__ == "CArgObject":       # C.byref(desc)
                a = a._obj
            args.append(_canon(a, spans))
        out.append([op.name, getattr(op.fn, "__name__", "torch_op"), args])
    return out
