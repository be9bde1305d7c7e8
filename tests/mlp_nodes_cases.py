"""Cases of the host layer under the six fused-MLP autograd nodes (``ops._FusedMLP``, ``_FusedMLPWide``,
``_FusedINEdgeWide``, ``ops_bf16.FusedMLP16``, ``FusedINEdge16``, ``HeadBCE16``), shared by the emulator and the GPU
tests.  ``case_launch_sequences`` pins WHICH C entries every node calls, in which order, forward and backward
(a recording proxy stands in for ``_capi._lib``); ``case_host_errors`` pins the errors and corner behaviours of the
host code.  The arithmetic itself is covered by tests/parity_cases.py and is not repeated here."""

import contextlib

import torch

import gnn_tracking_amd as G
from gnn_tracking_amd import _capi, dist as gdist, ops, ops_bf16 as B
from gnn_tracking_amd.interaction_network import InteractionNetwork

import fused_head_cases as F

N, E = 9, 33   # two 16-row fp32 tiles plus a row / one 32-row bf16 unit plus a row
MODES = ("fp32", "wide", "bf16")
_QUIET = ("gnntrk_last_error", "gnntrk_version")


class _Recorder:
    """Stands in for the bound library: every ``gnntrk_*`` entry called through it is listed by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("gnntrk_") or name in _QUIET:
            return fn

        def recorded(*a):
            self.calls.append(name[len("gnntrk_"):])
            return fn(*a)
        return recorded

    def take(self):
        calls, self.calls = self.calls, []
        return calls


@contextlib.contextmanager
def recording():
    old = _capi.load()
    rec = _Recorder(old)
    _capi._lib = rec
    try:
        yield rec
    finally:
        _capi._lib = old


def _rows(t, device, bf16):
    t = t.to(device)
    return (B.to_rows16(t) if bf16 else t.clone()).requires_grad_(True)


def _check(tag, tensors, like):
    """Finite, and shape / dtype of the tensor each one is the output or the gradient of."""
    for k, t in tensors.items():
        assert t is not None, f"{tag}: {k} is missing"
        shape, dtype = like[k]
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype, f"{tag}: {k} is {tuple(t.shape)} {t.dtype}"
        assert torch.isfinite(t.float()).all(), f"{tag}: {k} is not finite"


def _graph(device, seed=3):
    gen = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, N, (2, E), generator=gen).to(device)
    return gen, ops.graph_index(ei, N, cache=False)


def run_layer(device, mode, residue=None, *, no_grad=False, sinks=False):
    """One ``InteractionNetwork.forward_csr`` layer (``relu_in=True``) + backward.  ``residue``: None, "self" (the
    layer's own input, as in a residual stack) or "other" (a tensor of its own).  Returns ``(forward calls,
    backward calls, tensors)``."""
    bf16 = mode == "bf16"
    dn, de = (40, 40) if mode == "wide" else (5, 4)
    gen, gi = _graph(device)
    torch.manual_seed(0)
    net = InteractionNetwork(node_indim=dn, edge_indim=de, node_outdim=dn, edge_outdim=de, node_hidden_dim=40,
                             edge_hidden_dim=40).to(device)
    flat = gdist.FlatParameters(net, grad_sink=True) if sinks else None
    x0, e0, r0 = torch.randn(N, dn, generator=gen), torch.randn(E, de, generator=gen), torch.randn(N, dn, generator=gen)
    rx, re = torch.randn(N, dn, generator=gen).to(device), torch.randn(E, de, generator=gen).to(device)
    tag = f"layer {mode} residue={residue} no_grad={no_grad} sinks={sinks}"
    dt = torch.bfloat16 if bf16 else torch.float32
    with G.bf16_storage(bf16), recording() as rec:
        x, e = _rows(x0, device, bf16), _rows(e0, device, bf16)
        r = {None: None, "self": x, "other": _rows(r0, device, bf16)}[residue]
        rec.take()   # (the conversion passes of the inputs)
        with torch.set_grad_enabled(not no_grad):
            xo, eo = net.forward_csr(gi, x, e, relu_in=True, residue=r, alpha_residue=0.5)
        fwd = rec.take()
        out = {"x~": xo, "e~": eo}
        like = {"x~": ((N, dn), dt), "e~": ((E, de), dt)}
        if no_grad:
            assert not xo.requires_grad and not eo.requires_grad, tag
            _check(tag, out, like)
            return fwd, [], out
        loss = (xo.float() * rx).sum() + (eo.float() * re).sum()
        with ops.grad_sinks_armed() if sinks else contextlib.nullcontext():
            loss.backward()
        bwd = rec.take()
    out.update({"grad x": x.grad, "grad e": e.grad})
    like.update({"grad x": ((N, dn), dt), "grad e": ((E, de), dt)})
    if residue == "other":
        out["grad res"], like["grad res"] = r.grad, ((N, dn), dt)
    for k, v in net.named_parameters():
        out["grad " + k], like["grad " + k] = v.grad, (v.shape, torch.float32)
    _check(tag, out, like)
    if sinks:
        for p_ in flat.params:   # the gradients arrived in the bucket
            assert p_.grad.untyped_storage().data_ptr() == flat.grad.untyped_storage().data_ptr(), tag
    return fwd, bwd, {k: v.detach().clone() for k, v in out.items()}


def run_mlp(device, bf16, kind):
    """``fused_mlp`` + backward: ``kind`` "perm" (a "perm" segment, an identity segment, ``out_idx`` a permutation)
    or "sigmoid" (one identity segment, one output column, EPI_SIGMOID)."""
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(1)
    tag = f"fused_mlp {kind} bf16={bf16}"
    dt = torch.bfloat16 if bf16 else torch.float32
    with G.bf16_storage(bf16), recording() as rec:
        a, b = _rows(torch.randn(E, 5, generator=gen), device, bf16), _rows(torch.randn(E, 4, generator=gen), device, bf16)
        rec.take()
        if kind == "perm":
            mlp = G.MLP(9, 4, 40, L=3).to(device)
            idx = torch.randperm(E, generator=gen).int().to(device)
            oidx = torch.randperm(E, generator=gen).int().to(device)
            segs, kw, odt = [ops.Seg(a, idx, False, "perm"), ops.Seg(b)], dict(out_idx=oidx), dt
        else:
            mlp = G.MLP(9, 1, 40, L=3).to(device)
            segs, kw, odt = [ops.Seg(a), ops.Seg(b)], dict(epilogue=_capi.EPI_SIGMOID, ca=0.0, cb=1.0), torch.float32
        out = mlp.fused(segs, **kw)
        fwd = rec.take()
        ro = torch.randn(*out.shape, generator=gen).to(device)
        (out.float() * ro).sum().backward()
        bwd = rec.take()
    got = {"out": out, "grad a": a.grad, "grad b": b.grad}
    like = {"out": ((E, mlp.out_dim), odt), "grad a": ((E, 5), dt), "grad b": ((E, 4), dt)}
    for k, v in mlp.named_parameters():
        got["grad " + k], like["grad " + k] = v.grad, (v.shape, torch.float32)
    _check(tag, got, like)
    return fwd, bwd, {k: v.detach().clone() for k, v in got.items()}


def head_data(device):
    gen = torch.Generator().manual_seed(17)
    return G.Data(x=torch.randn(N, 6, generator=gen).to(device), edge_index=torch.randint(0, N, (2, E), generator=gen).to(device),
                  edge_attr=torch.randn(E, 4, generator=gen).to(device), y=(torch.rand(E, generator=gen) < 0.5).to(device),
                  pt=(torch.rand(N, generator=gen) + 0.1).to(device))


def run_head(device, deferred):
    """One ``TrackingModule.backward_step`` of the edge classifier in bf16 storage, the head deferred into its
    backward launch (``HeadBCE16``) or not.  The forward part ends where ``training_step`` returns the loss."""
    data = head_data(device)
    mod = F.make_module(device, data)
    inner = mod._loss
    tag = f"backward_step deferred={deferred}"
    keep = {}
    mod.model.register_forward_hook(lambda m, i, out: keep.update(out=out))
    with F.deferral(deferred), recording() as rec:
        parts = {}

        def marked(d):
            loss = inner(d)
            parts["fwd"] = rec.take()
            parts["node"] = type(loss.grad_fn).__name__
            return loss
        mod._loss = marked
        ops.clear_graph_index_cache()
        mod.zero_grad()
        rec.take()
        loss = mod.backward_step(data)
        bwd = rec.take()
    assert parts["node"].startswith("HeadBCE16") == deferred, f"{tag}: the loss came from {parts['node']}"
    # (the weights of a deferred head exist once the backward launch has written them)
    got = {"loss": loss.reshape(()), "W": keep["out"]["W"].csr}
    like = {"loss": ((), torch.float32), "W": ((E,), torch.float32)}
    for k, v in mod.model.named_parameters():
        if v.grad is not None:
            got["grad " + k], like["grad " + k] = v.grad, (v.shape, torch.float32)
    assert len(got) > 2, tag
    _check(tag, got, like)
    return parts["fwd"], bwd, {k: v.detach().clone() for k, v in got.items()}


def configurations():
    """name -> callable(device) returning ``(forward calls, backward calls, tensors)``."""
    cfg = {}
    for mode in MODES:
        for residue in (None, "self", "other"):
            cfg[f"layer {mode} residue={residue}"] = lambda d, m=mode, r=residue: run_layer(d, m, r)
        cfg[f"layer {mode} sinks"] = lambda d, m=mode: run_layer(d, m, "self", sinks=True)
    cfg["layer wide no_grad"] = lambda d: run_layer(d, "wide", "self", no_grad=True)
    for bf16 in (False, True):
        for kind in ("perm", "sigmoid"):
            cfg[f"fused_mlp {kind} {'bf16' if bf16 else 'fp32'}"] = lambda d, b=bf16, k=kind: run_mlp(d, b, k)
    cfg["head deferred"] = lambda d: run_head(d, True)
    cfg["head not deferred"] = lambda d: run_head(d, False)
    return cfg


#: name -> (forward entries, backward entries), as recorded on the tree before the nodes shared their host path
EXPECTED = {
 'fused_mlp perm bf16': (['mlp_forward_bf16'],
                         ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'permute_rows_bf16']),
 'fused_mlp perm fp32': (['mlp_forward'], ['mlp_backward_workspace_bytes', 'mlp_backward', 'permute_rows']),
 'fused_mlp sigmoid bf16': (['mlp_forward_bf16'], ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16']),
 'fused_mlp sigmoid fp32': (['mlp_forward'], ['mlp_backward_workspace_bytes', 'mlp_backward']),
 'head deferred': (['graph_index_workspace_bytes_carry', 'graph_index_build_carry', 'rows_to_bf16',
                    'mlp_forward_bf16', 'mlp_forward_bf16', 'mlp_forward_bf16', 'segment_sum_bf16',
                    'mlp_forward_bf16', 'mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16',
                    'mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16'],
                   ['mlp_backward_bf16_bce_supported', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16_bce',
                    'bce_workspace_bytes', 'bce_csr', 'segment_sum_bf16', 'segment_sum_bf16_add',
                    'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'mlp_backward_bf16_workspace_bytes',
                    'mlp_backward_bf16', 'segment_sum_bf16_add', 'segment_sum_bf16_add',
                    'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'mlp_backward_bf16_max_terms',
                    'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16_add',
                    'segment_sum_bf16_add', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                    'mlp_backward_bf16_max_terms', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                    'segment_sum_bf16_add', 'segment_sum_bf16_add', 'mlp_backward_bf16_workspace_bytes',
                    'mlp_backward_bf16', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16']),
 'head not deferred': (['graph_index_workspace_bytes_carry', 'graph_index_build_carry', 'rows_to_bf16',
                        'mlp_forward_bf16', 'mlp_forward_bf16', 'mlp_forward_bf16', 'segment_sum_bf16',
                        'mlp_forward_bf16', 'mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16',
                        'mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16', 'mlp_forward_bf16',
                        'bce_workspace_bytes', 'bce_csr'],
                       ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16',
                        'segment_sum_bf16_add', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                        'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16_add',
                        'segment_sum_bf16_add', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                        'mlp_backward_bf16_max_terms', 'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                        'segment_sum_bf16_add', 'segment_sum_bf16_add', 'mlp_backward_bf16_workspace_bytes',
                        'mlp_backward_bf16', 'mlp_backward_bf16_max_terms', 'mlp_backward_bf16_workspace_bytes',
                        'mlp_backward_bf16', 'segment_sum_bf16_add', 'segment_sum_bf16_add',
                        'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'mlp_backward_bf16_workspace_bytes',
                        'mlp_backward_bf16']),
 'layer bf16 residue=None': (['mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16'],
                             ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                              'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16_add',
                              'segment_sum_bf16_add']),
 'layer bf16 residue=other': (['mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16'],
                              ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                               'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16_add',
                               'segment_sum_bf16_add']),
 'layer bf16 residue=self': (['mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16'],
                             ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16',
                              'mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'segment_sum_bf16_add',
                              'segment_sum_bf16_add']),
 'layer bf16 sinks': (['mlp_forward_bf16', 'segment_sum_bf16', 'mlp_forward_bf16'],
                      ['mlp_backward_bf16_workspace_bytes', 'mlp_backward_bf16', 'mlp_backward_bf16_workspace_bytes',
                       'mlp_backward_bf16', 'segment_sum_bf16_add', 'segment_sum_bf16_add']),
 'layer fp32 residue=None': (['mlp_forward', 'segment_sum', 'mlp_forward'],
                             ['mlp_backward_workspace_bytes', 'mlp_backward', 'permute_rows',
                              'mlp_backward_workspace_bytes', 'mlp_backward', 'segment_sum', 'segment_sum']),
 'layer fp32 residue=other': (['mlp_forward', 'segment_sum', 'mlp_forward'],
                              ['mlp_backward_workspace_bytes', 'mlp_backward', 'axpby', 'permute_rows',
                               'mlp_backward_workspace_bytes', 'mlp_backward', 'segment_sum', 'segment_sum']),
 'layer fp32 residue=self': (['mlp_forward', 'segment_sum', 'mlp_forward'],
                             ['mlp_backward_workspace_bytes', 'mlp_backward', 'axpby', 'permute_rows',
                              'mlp_backward_workspace_bytes', 'mlp_backward', 'segment_sum', 'segment_sum']),
 'layer fp32 sinks': (['mlp_forward', 'segment_sum', 'mlp_forward'],
                      ['mlp_backward_workspace_bytes', 'mlp_backward', 'axpby', 'permute_rows',
                       'mlp_backward_workspace_bytes', 'mlp_backward', 'segment_sum', 'segment_sum']),
 'layer wide no_grad': (['mlp_wide_forward_workspace_bytes', 'mlp_forward_wide', 'segment_sum',
                         'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide'],
                        []),
 'layer wide residue=None': (['mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide',
                              'segment_sum', 'mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes',
                              'mlp_forward_wide'],
                             ['mlp_wide_backward_workspace_bytes', 'mlp_backward_wide',
                              'mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'segment_sum',
                              'segment_sum']),
 'layer wide residue=other': (['mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide',
                               'segment_sum', 'mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes',
                               'mlp_forward_wide'],
                              ['mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'axpby',
                               'mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'segment_sum',
                               'segment_sum']),
 'layer wide residue=self': (['mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide',
                              'segment_sum', 'mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes',
                              'mlp_forward_wide'],
                             ['mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'axpby',
                              'mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'segment_sum',
                              'segment_sum']),
 'layer wide sinks': (['mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide', 'segment_sum',
                       'mlp_wide_hidden_pad', 'mlp_wide_forward_workspace_bytes', 'mlp_forward_wide'],
                      ['mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'axpby',
                       'mlp_wide_backward_workspace_bytes', 'mlp_backward_wide', 'segment_sum', 'segment_sum']),
}


def case_launch_sequences(device):
    cfg = configurations()
    assert cfg.keys() == EXPECTED.keys()
    got = {}
    for name, run in cfg.items():
        fwd, bwd, got[name] = run(device)
        assert fwd == EXPECTED[name][0], f"{name}: forward launches {fwd}"
        assert bwd == EXPECTED[name][1], f"{name}: backward launches {bwd}"
    assert "mlp_wide_hidden_pad" not in EXPECTED["layer wide no_grad"][0]   # (no activations kept for a backward)
    assert "mlp_backward_bf16_bce" in EXPECTED["head deferred"][1]
    # gradients that arrive through the sinks are the gradients the node returns without them - once, not twice
    for mode in MODES:
        a, b = got[f"layer {mode} sinks"], got[f"layer {mode} residue=self"]
        for k in a:
            assert torch.equal(a[k], b[k]), f"layer {mode}: {k} through the gradient sinks differs"
    return got


# ------------------------------------------------------------------------------------------ host errors
EH = 17   # rows of the error cases: one 16-row tile plus a row


def _mlp_for(mode, in_dim, out_dim, device):
    """An MLP whose shape selects the node of ``mode``: hidden 80 is beyond the register-resident fp32 kernels."""
    return G.MLP(in_dim, out_dim, 80 if mode == "wide" else 40, L=3).to(device)


class _Drop(torch.autograd.Function):
    """Identity whose backward hands NO gradient to its input (an undefined gradient, as from an unused output)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return None


def case_host_errors(device):
    import types

    import pytest

    for mode in MODES:
        bf16 = mode == "bf16"
        gen = torch.Generator().manual_seed(23)
        torch.manual_seed(2)
        with G.bf16_storage(bf16):
            mlp = _mlp_for(mode, 9, 4, device)
            idx = torch.randint(0, EH, (EH,), generator=gen).int().to(device)
            perm = torch.randperm(EH, generator=gen).int().to(device)

            def rows(n, d):
                return _rows(torch.randn(n, d, generator=gen), device, bf16)

            def go(segs, m=mlp, **kw):
                out = m.fused(segs, **kw)
                node = type(out.grad_fn).__name__
                want = {"fp32": "_FusedMLPBackward", "wide": "_FusedMLPWideBackward", "bf16": "FusedMLP16Backward"}[mode]
                assert node == want, f"{mode}: the node is {node}"
                return out

            # a gathered segment without a fold rule, its gradient wanted
            out = go([ops.Seg(rows(EH, 5), idx, False, None), ops.Seg(rows(EH, 4))])
            with pytest.raises(RuntimeError, match="reduce"):
                out.float().sum().backward()
            # segment widths that are not the first layer's input width
            with pytest.raises(AssertionError, match="Expected feature dimension"):
                _mlp_for(mode, 10, 4, device).fused([ops.Seg(rows(EH, 5)), ops.Seg(rows(EH, 4))])
            # a "perm" segment over a source with more rows than the launch
            out = go([ops.Seg(rows(EH + 3, 5), perm, False, "perm"), ops.Seg(rows(EH, 4))])
            with pytest.raises(RuntimeError, match="perm"):
                out.float().sum().backward()
            # an identity segment over a source with more rows than the launch
            big, b = rows(EH + 3, 5), rows(EH, 4)
            ro = torch.randn(EH, 4, generator=gen).to(device)
            out = go([ops.Seg(big), ops.Seg(b)], n_rows=EH)
            if mode == "fp32":   # the register-resident backward: a gradient of the source's height, zero below
                (out * ro).sum().backward()
                cut = big.detach()[:EH].clone().requires_grad_(True)
                (go([ops.Seg(cut), ops.Seg(b)], n_rows=EH) * ro).sum().backward()
                assert tuple(big.grad.shape) == (EH + 3, 5) and tuple(cut.grad.shape) == (EH, 5)
                assert torch.equal(big.grad[:EH], cut.grad) and not bool(big.grad[EH:].any())
                assert bool(cut.grad.any())
            else:
                with pytest.raises(RuntimeError, match="identity segments must have n_rows rows"):
                    (out.float() * ro).sum().backward()
            # segment count and rank
            lin = mlp.linears()
            wb = ([m.weight for m in lin], [m.bias for m in lin])
            with pytest.raises(ValueError, match="segments supported"):
                ops.fused_mlp([], *wb)
            with pytest.raises(ValueError, match="segments supported"):
                ops.fused_mlp([ops.Seg(rows(EH, 1)) for _ in range(_capi.MAX_SEGS + 1)], *wb)
            with pytest.raises(ValueError, match="2-D"):
                ops.fused_mlp([ops.Seg(rows(EH, 9)[:, 0])], *wb)

    # the relational + aggregation nodes without any upstream gradient
    gen, gi = _graph(device)
    with pytest.raises(RuntimeError, match="without upstream gradients"):
        B.FusedINEdge16.backward(types.SimpleNamespace(gi=gi, stash=None, node_stash=None), None, None)
    torch.manual_seed(3)
    net = InteractionNetwork(node_indim=40, edge_indim=40, node_outdim=40, edge_outdim=40).to(device)
    x, e = _rows(torch.randn(N, 40, generator=gen), device, False), _rows(torch.randn(E, 40, generator=gen), device, False)
    lin = net.relational_model.linears()
    with recording() as rec:
        et, aggr = ops.in_edge_wide([ops.Seg(x, gi.tgt, True, ("tgt", gi)), ops.Seg(x, gi.src, True, ("src", gi)),
                                     ops.Seg(e, None, True)], [m.weight for m in lin], [m.bias for m in lin], gi, E)
        assert type(et.grad_fn).__name__ == "_FusedINEdgeWideBackward"
        rec.take()
        grads = torch.autograd.grad(_Drop.apply(et).sum() + _Drop.apply(aggr).sum(),
                                    [x, e] + list(net.relational_model.parameters()), allow_unused=True)
        assert all(g is None for g in grads) and rec.take() == []
