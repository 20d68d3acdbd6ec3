"""The A-NeRF (nerf_type = nerf) training step on the HIP path: `danbo_anerf_train_step` (forward + the two rgb losses + backward of
one batch behind one C call, csrc/k_anerf_train.hip) and `danbo_adam_step` on flat parameter / gradient buffers -- the A-NeRF
counterpart of core/train_engine.py, whose flat-buffer, Adam-state, random-stream and HIP-graph machinery it inherits.

Reference: Trainer.train_batch (core/trainer.py:257-302) with NeRF.forward (core/networks/nerf.py:107-122,176-209,222-279) and the
cutoff encoders (core/cutoff_embedder.py:151-214).  Every dense W-wide layer runs on k_linear16 both ways and k_dw16; the encoders,
the view branch, the colour head, the composites and every adjoint are this library's kernels: there is no torch / rocBLAS
kernel in the step (round 5 trained A-NeRF through autograd with library GEMMs for the heads and the view products).
"""
import ctypes

import torch

from . import _hip
from ._hip import ptr
from .train_engine import DanboTrainEngine, unsupported_options


def _names(net):
    D = len(net.pts_linears)
    names = ([f"pts_linears.{i}.weight" for i in range(D)] + [f"pts_linears.{i}.bias" for i in range(D)]
             + ["alpha_linear.weight", "alpha_linear.bias", "feature_linear.weight", "feature_linear.bias", "views_linears.0.weight",
                "views_linears.0.bias", "rgb_linear.weight", "rgb_linear.bias"])
    if net.use_framecode:
        names.append("framecodes.codes.weight")
    return names


def supported(args, caster):
    """-> None if danbo_anerf_train_step covers this configuration, else the reason (the caller then uses the autograd path)"""
    reason = unsupported_options(args, caster, 'NeRF')
    if reason is not None:
        return reason
    net = caster.network
    if args.N_importance <= 0 or args.N_samples + args.N_importance > 256 or args.N_samples < 3:
        return 'sampling settings'
    try:
        cfg = net.engine_config()
    except Exception as e:       # an encoder combination the A-NeRF kernels do not cover
        return f'engine_config: {e}'
    D, W, VW = len(net.pts_linears), net.W, net.views_linears[0].weight.shape[0]
    if net.feature_linear.weight.shape[0] != W:
        return 'feature_linear width != W'          # (the reference: 2 view_W = W)
    skips = list(net.skips)
    if not (2 <= D <= _hip.ANERF_MAX_D) or W % 4 or W > 508 or VW % 4 or VW > 256 or len(net.views_linears) != 1:
        return 'MLP shape'
    if len(skips) > 1 or (skips and not 0 <= skips[0] <= D - 2):
        return f'skips {skips}'
    sd = dict(net.named_parameters())
    for n in _names(net):
        if n not in sd:
            return f'missing parameter {n}'
        if not sd[n].requires_grad:
            return f'{n} is frozen'
    extra = {n for n, p in sd.items() if p.requires_grad} - set(_names(net))
    if extra:
        return f'trainable parameters outside the fused step: {sorted(extra)}'
    if not torch.equal(net.pe_fn.cutoff_dist, net.dirs_pe_fn.cutoff_dist):
        return 'distance and view cutoffs differ'
    return None


class AnerfTrainEngine(DanboTrainEngine):
    phases = 1      # the whole step is one phase: a split step leaves nothing for finish_backward()

    def __init__(self, args, caster, optimizer):
        order = _names(caster.network)
        self._init_flat(args, caster, optimizer, order, order, [])
        self._init_state()
        # tau as a DEVICE scalar at a fixed address: update_tau REPLACES the module's buffer every step (core/cutoff_embedder.py) and a
        # captured graph holds pointers -- forward_backward copies the current value in front of every step
        self._tau = torch.zeros(1, device=self.device, dtype=torch.float32)

    def _model(self):
        if self._model_struct is not None:
            return self._model_struct
        net, args = self.net, self.args
        m = _hip.DanboAnerfTrainModel()
        cfg = net.engine_config()
        D = len(net.pts_linears)
        pp = lambda n: self.flat_p.data_ptr() + 4 * self.offsets[n]  # noqa: E731
        gp = lambda n: self.flat_g.data_ptr() + 4 * self.offsets[n]  # noqa: E731
        m.D, m.W, m.VW = D, net.W, net.views_linears[0].weight.shape[0]
        skips = list(net.skips)
        m.skip = skips[0] if skips else -1
        m.L, m.L_view = int(cfg["multires"]), int(cfg["multires_views"])
        for i in range(D):
            m.pts_w[i], m.pts_b[i] = pp(f"pts_linears.{i}.weight"), pp(f"pts_linears.{i}.bias")
            m.g_pts_w[i], m.g_pts_b[i] = gp(f"pts_linears.{i}.weight"), gp(f"pts_linears.{i}.bias")
        for f, n in (("alpha_w", "alpha_linear.weight"), ("alpha_b", "alpha_linear.bias"), ("feature_w", "feature_linear.weight"),
                     ("feature_b", "feature_linear.bias"), ("views_w", "views_linears.0.weight"), ("views_b", "views_linears.0.bias"),
                     ("rgb_w", "rgb_linear.weight"), ("rgb_b", "rgb_linear.bias")):
            setattr(m, f, pp(n))
            setattr(m, "g_" + f, gp(n))
        if net.use_framecode:
            m.n_codes, m.code_size = net.framecodes.codes.weight.shape
            m.codes, m.g_codes = pp("framecodes.codes.weight"), gp("framecodes.codes.weight")
        want = m.W + 72 * (1 + 2 * m.L_view) + m.code_size
        if net.views_linears[0].weight.shape[1] != want or net.pts_linears[0].weight.shape[1] != 24 * (1 + 2 * m.L) + 72:
            raise RuntimeError("A-NeRF layer widths do not match the cutoff encoders (reldist + reldir density inputs, relray view inputs)")
        m.g_flat, m.n_flat = self.flat_g.data_ptr(), self.flat_g.numel()
        keep = self._buffers
        keep['align'] = self.caster.transforms[0].to(self.device).float().contiguous()
        keep['cutoff'] = net.pe_fn.cutoff_dist.detach().to(self.device).float().contiguous()
        m.align, m.cutoff, m.tau = keep['align'].data_ptr(), keep['cutoff'].data_ptr(), self._tau.data_ptr()
        m.loss_mse, m.use_background = int(args.loss_fn == 'MSE'), int(bool(args.use_background))
        m.density_scale = float(args.density_scale)
        m.rgb_loss_coef, m.coarse_weight = float(args.rgb_loss_coef), float(args.coarse_weight)
        self._model_struct = m
        return m

    # ------------------------------------------------------------------ the C entry points
    def _c_workspace(self, m, R, G, S, Sf, chunk):
        return _hip.lib().danbo_anerf_train_workspace(ctypes.byref(m), R, G, S, Sf, chunk)

    def _c_step(self, m, bt, o, phase, stream):
        _hip.call("danbo_anerf_train_step", ctypes.byref(m), ctypes.byref(bt), ctypes.byref(o), ptr(self._ws), self._ws.numel(), stream)

    def forward_backward(self, *a, **k):
        tau, tau_v = float(self.net.pe_fn.tau), float(self.net.dirs_pe_fn.tau)
        if tau != tau_v:
            raise NotImplementedError("pe_fn.tau != dirs_pe_fn.tau: the shared cutoff weight no longer applies")
        self._tau.copy_(self.net.pe_fn.tau.detach().reshape(1).to(self.device, torch.float32))
        out = super().forward_backward(*a, **k)
        c = out.get('counts')      # the A-NeRF step has no row counters (every sample is evaluated): zeros, once per static buffer
        if c is not None and (not self.outputs_static or getattr(self, '_counts_graph', None) is not self.graph):
            c.zero_()
            self._counts_graph = self.graph
        return out

    def grad_buckets(self):
        """(finished after phase 1, finished after phase 2): the whole flat gradient is final after the one phase of this step"""
        return self.flat_g[:self.n_train], self.flat_g[:0]

    def workspace_view(self, R, G, S, Sf):
        """device views of the last step's sampling decisions (z_coarse [R,S], z_fine [R,Sf], z_sorted, order [R,S+Sf])"""
        v = _hip.DanboTrainView()
        _hip.call("danbo_anerf_train_workspace_view", ctypes.byref(self._model()), R, G, S, Sf, R, ptr(self._ws), ctypes.byref(v))
        return v
