"""Feed-forward policy on the recent CGM, insulin and meal history, host form.

The reference ships hand-written controllers only (``simglucose/controller/pid_ctrller.py``,
``basal_bolus_ctrller.py``); its gym users put a learned network in the same slot.  ``MLPController`` is that network
with the reference's controller surface (``policy`` / ``reset``, so it drops into ``SimObj``), and the host
restatement of what ``BatchedT1DSimEnv.rollout_mlp`` evaluates inside the kernel (``t1d_mlp`` / ``t1d_rollout_mlp``
in ``include/t1d.h``, ``csrc/t1d_policy.hpp``) for a whole batch:

    features (F = 2 H + 3):  (CGM[-k] - cgm_mean) cgm_scale, k = 0 .. H-1      CGM[0] = the current observation
                             INS[-1-k] ins_scale,           k = 0 .. H-1      mean pump output of earlier steps, U/min
                             prev_meal cho_scale                               mean announced CHO of the last step, g/min
                             sin(2 pi m / 1440), cos(2 pi m / 1440)            m = minute of day at the start of the step
    layers:                  x <- act(W x + b), the last one without activation and of width 1
    basal = out_scale g(y) + out_bias,  g = identity or logistic;  bolus = 0, or with meal_bolus= the meal bolus below

The kernel accumulates ``b[o]`` first and then ``W[o][j] x[j]`` for j ascending with one fused multiply-add each;
``forward(..., ordered=True)`` adds in that order, ``ordered=False`` is a plain ``torch.matmul``.
``BatchedT1DSimEnv.collect_mlp`` adds ``sigma * eps`` to the last layer's output before ``g``; ``log_prob`` is the
density of that sample.

``meal_bolus=`` makes the policy a hybrid closed loop: the network commands the basal rate and a bolus calculator doses each
announced meal by ``BBController``'s rule (``basal_bolus_ctrller.py``), from the words a step already holds:

    corr  = CGM[0] > 150 ? (CGM[0] - target) / CF : 0
    bolus = prev_meal > 0 ? ((prev_meal st) / CR + corr) / st : 0        U/min, st = the sensor's sample time

``rollout_mlp``, ``collect_mlp`` and ``rollout_mlp_dopri5`` then run the ``*_bolus`` entry points of ``include/t1d.h``, which form
that bolus inside the kernel beside the network's basal; ``BatchedT1DSimEnv.policy_bolus`` gives it for a ``step()`` loop.  The
density, ``eps`` and the features are untouched: the bolus is a deterministic function of the state.

``relative_to="basal"`` makes the output a multiple of the patient's own basal rate, ``basal = (out_scale g(y) + out_bias) basal_i``
with ``basal_i = u2ss BW / 6000`` (``BBController``'s basal): the ``*_rel`` entry points read ``scale[i] = out_scale basal_i`` and
``bias[i] = out_bias basal_i`` per env, so one weight set serves a cohort whose basal rates differ by a factor of four.  Noise is
added before ``g`` as ever; the density lives in ``y`` and the trainer's calls are untouched.
"""
import math

import torch

from .base import Action, Controller
from .basal_bolus_ctrller import BBController

MAX_HISTORY, MAX_LAYERS, MAX_WIDTH = 12, 4, 32
_HIDDEN = {"tanh": 0, "relu": 1}
_OUTPUT = {"identity": 0, "logistic": 1}


class MLPController(Controller):
    """layers: list of (W, b) with W [out, in] and b [out] -- or W [P, out, in] and b [P, out] for a stack of P weight
    sets (the multi-policy roll-out: env i uses set i // (n // P)).  The first layer takes F = 2 history + 3 inputs, the
    last has one output.  Weights are kept as float64 CPU tensors.  meal_bolus: None (the policy commands a basal rate and
    nothing else), a target in mg/dL, or a BBController whose target is used -- kept as a BBController in .meal_bolus.
    relative_to: None (out_scale and out_bias are U/min) or "basal" (they are multiples of the patient's basal rate)."""

    def __init__(self, layers, history=4, hidden="tanh", output="identity", cgm_mean=140.0, cgm_scale=0.01,
                 ins_scale=10.0, cho_scale=0.1, out_scale=1.0, out_bias=0.0, meal_bolus=None, relative_to=None):
        if relative_to not in (None, "basal"):
            raise ValueError("relative_to must be None or 'basal'")
        self.relative_to = relative_to
        if meal_bolus is not None and not isinstance(meal_bolus, BBController):
            if isinstance(meal_bolus, bool) or not isinstance(meal_bolus, (int, float)) or not math.isfinite(meal_bolus):
                raise ValueError("meal_bolus must be None, a target in mg/dL or a BBController")
            meal_bolus = BBController(target=meal_bolus)
        self.meal_bolus = meal_bolus
        history = int(history)
        if not 1 <= history <= MAX_HISTORY:
            raise ValueError("history must be in [1, %d]" % MAX_HISTORY)
        if hidden not in _HIDDEN:
            raise ValueError("hidden must be 'tanh' or 'relu'")
        if output not in _OUTPUT:
            raise ValueError("output must be 'identity' or 'logistic'")
        layers = list(layers)
        if not 1 <= len(layers) <= MAX_LAYERS:
            raise ValueError("an MLPController has 1 to %d layers" % MAX_LAYERS)
        self.history, self.hidden, self.output = history, hidden, output
        self.cgm_mean, self.cgm_scale, self.ins_scale = float(cgm_mean), float(cgm_scale), float(ins_scale)
        self.cho_scale, self.out_scale, self.out_bias = float(cho_scale), float(out_scale), float(out_bias)
        self.W, self.b = [], []
        n_in, npol = self.n_features, None
        for W, b in layers:
            W = torch.as_tensor(W).detach().to("cpu", torch.float64)
            b = torch.as_tensor(b).detach().to("cpu", torch.float64)
            if W.dim() == 2:
                W, b = W.unsqueeze(0), b.unsqueeze(0)
            if W.dim() != 3 or b.dim() != 2 or b.shape != W.shape[:2]:
                raise ValueError("a layer is (W [out, in], b [out]) or (W [P, out, in], b [P, out])")
            if npol is None:
                npol = W.shape[0]
            if W.shape[0] != npol:
                raise ValueError("every layer must hold the same number of weight sets")
            if W.shape[2] != n_in:
                raise ValueError("layer %d takes %d inputs, the one before it gives %d" % (len(self.W), W.shape[2], n_in))
            if not 1 <= W.shape[1] <= MAX_WIDTH:
                raise ValueError("layer widths must be in [1, %d]" % MAX_WIDTH)
            self.W.append(W.contiguous()); self.b.append(b.contiguous())
            n_in = W.shape[1]
        if n_in != 1:
            raise ValueError("the last layer must have one output")
        self.n_policies = int(npol)
        self._dev = {}
        self.reset()

    # ------------------------------------------------------------------ construction / flat form
    @property
    def n_features(self):
        return 2 * self.history + 3

    @property
    def widths(self):
        return [int(W.shape[1]) for W in self.W]

    @staticmethod
    def count_params(history, widths):
        n_in, total = 2 * int(history) + 3, 0
        for w in widths:
            total += w * (n_in + 1)
            n_in = w
        return total

    @classmethod
    def from_torch(cls, net, history=4, **kw):
        """From an ``nn.Sequential`` of Linear layers with Tanh or ReLU between them and an optional Sigmoid at the end."""
        from torch import nn
        layers, acts, output = [], set(), "identity"
        mods = list(net)
        for k, m in enumerate(mods):
            if isinstance(m, nn.Linear):
                if m.bias is None:
                    raise ValueError("Linear layers need a bias")
                layers.append((m.weight, m.bias))
            elif isinstance(m, nn.Sigmoid) and k == len(mods) - 1:
                output = "logistic"
            elif isinstance(m, nn.Tanh):
                acts.add("tanh")
            elif isinstance(m, nn.ReLU):
                acts.add("relu")
            else:
                raise ValueError("unsupported module %r" % (m,))
        if len(acts) > 1:
            raise ValueError("one hidden activation for the whole net")
        kw.setdefault("hidden", acts.pop() if acts else "tanh")
        kw.setdefault("output", output)
        return cls(layers, history=history, **kw)

    @classmethod
    def from_flat(cls, params, widths, history=4, **kw):
        """Inverse of flat_params(): params [n_params] or [P, n_params]."""
        params = torch.as_tensor(params).detach().to("cpu", torch.float64)
        if params.dim() == 1:
            params = params.unsqueeze(0)
        if params.dim() != 2 or params.shape[1] != cls.count_params(history, widths):
            raise ValueError("params must have %d entries per weight set" % cls.count_params(history, widths))
        layers, n_in, at = [], 2 * int(history) + 3, 0
        for w in widths:
            W = params[:, at:at + w * n_in].reshape(-1, w, n_in); at += w * n_in
            b = params[:, at:at + w]; at += w
            layers.append((W, b))
            n_in = w
        return cls(layers, history=history, **kw)

    def flat_params(self):
        """-> float64 [P, n_params]: per weight set the layers in order, each as row-major W[out][in] then b[out]
        (the layout of t1d_mlp.params)."""
        P = self.n_policies
        return torch.cat([torch.cat([W.reshape(P, -1), b], dim=1) for W, b in zip(self.W, self.b)], dim=1).contiguous()

    def device_params(self, device, dtype):
        """flat_params() on `device` in `dtype`, uploaded once and kept (rollout_mlp calls this for every launch).  After
        editing W or b in place call invalidate()."""
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = self.flat_params().to(device=device, dtype=dtype).contiguous()
        return self._dev[key]

    def invalidate(self):
        """forget the uploaded copies of the weights"""
        self._dev = {}

    def fill_struct(self, p):
        """the scalar fields of a _lib.Mlp"""
        p.history, p.n_layers = self.history, len(self.W)
        for k in range(4):
            p.width[k] = self.widths[k] if k < len(self.W) else 0
        p.hidden_act, p.out_act = _HIDDEN[self.hidden], _OUTPUT[self.output]
        p.cgm_mean, p.cgm_scale, p.ins_scale, p.cho_scale = self.cgm_mean, self.cgm_scale, self.ins_scale, self.cho_scale
        p.out_scale, p.out_bias = self.out_scale, self.out_bias

    # ------------------------------------------------------------------ batched host restatement
    def features(self, cgm_hist, ins_hist, prev_meal, minute):
        """cgm_hist [H, n] (row k = CGM[-k]), ins_hist [H, n] (row k = INS[-1-k]), prev_meal [n], minute [n] (integer minute
        of day at the start of the step, or minutes since midnight of any day) -> features [F, n] in the kernel's order."""
        dt = cgm_hist.dtype
        ang = (torch.as_tensor(minute, device=cgm_hist.device) % 1440).to(dt) * (2.0 * math.pi / 1440.0)
        ang = ang.expand(cgm_hist.shape[1])
        return torch.cat([(cgm_hist - self.cgm_mean) * self.cgm_scale, ins_hist * self.ins_scale,
                          (prev_meal * self.cho_scale).unsqueeze(0), torch.sin(ang).unsqueeze(0), torch.cos(ang).unsqueeze(0)], dim=0)

    @staticmethod
    def shift(cgm_hist, ins_hist, cgm, insulin):
        """The window shift after a step: the new observation and the step's mean pump output enter row 0 (in place)."""
        cgm_hist[1:] = cgm_hist[:-1].clone(); cgm_hist[0] = cgm
        ins_hist[1:] = ins_hist[:-1].clone(); ins_hist[0] = insulin

    def pre_output(self, feat, ordered=False):
        """feat [F, n] -> y [n]: the last layer's output, before the output function (forward without out_scale g(.) +
        out_bias) -- the word collect_mlp adds sigma * eps to.  With P weight sets env i uses set i // (n // P).  ordered:
        accumulate bias first, then input by input in ascending order, as the kernel does; otherwise torch.matmul."""
        P, n = self.n_policies, feat.shape[1]
        if n % P:
            raise ValueError("%d envs do not split into %d weight sets" % (n, P))
        x = feat.reshape(feat.shape[0], P, n // P).permute(1, 0, 2)            # [P, in, n / P]
        for k, (W, b) in enumerate(zip(self.W, self.b)):
            W, b = W.to(feat.device, feat.dtype), b.to(feat.device, feat.dtype)
            if ordered:
                acc = b.unsqueeze(2).expand(P, W.shape[1], n // P).clone()
                for j in range(W.shape[2]):
                    acc = torch.addcmul(acc, W[:, :, j:j + 1], x[:, j:j + 1, :])
                x = acc
            else:
                x = torch.matmul(W, x) + b.unsqueeze(2)
            if k + 1 < len(self.W):
                x = torch.tanh(x) if self.hidden == "tanh" else torch.relu(x)
        return x.reshape(n)

    def forward(self, feat, ordered=False, ref=None):
        """feat [F, n] -> basal [n], U/min: out_scale g(pre_output(feat, ordered)) + out_bias, times ref [n] when given
        (relative_to="basal": each env's basal rate)."""
        y = self.pre_output(feat, ordered)
        g = torch.sigmoid(y) if self.output == "logistic" else y
        u = self.out_scale * g + self.out_bias
        return u if ref is None else u * ref

    def grad_reference(self, feat_rows, coef, params=None, info=False):
        """What t1d_mlp_grad (controller.mlp_pre_output's backward) computes, in plain torch and fp64 on the device of
        feat_rows: feat_rows [K, F, n], coef [K, n] = dL/dy of every sample -> grad [P, n_params] in the layout of
        flat_params(), grad[p][q] = sum over the K rows and the envs of policy p of coef * dy / dparams[p][q], by a manual
        back-propagation (tanh' = 1 - a^2, relu' = a > 0) -- no autograd graph.  params: [P, n_params] to use instead of this
        controller's weights (taken to fp64 as they are).  info=True: -> (grad, dict) with "scale" [P, n_params], S = sum of
        |coef * dy / dparam| per parameter, the size a rounding error bound is stated in, and "min_abs_pre", the smallest
        |pre-activation| of any hidden unit (how far a relu net is from a kink)."""
        K, F, n = feat_rows.shape
        P = self.n_policies
        if F != self.n_features or n % P or tuple(coef.shape) != (K, n):
            raise ValueError("grad_reference: feat_rows [K, %d, n] and coef [K, n] with n a multiple of %d" % (self.n_features, P))
        dev, f64 = feat_rows.device, torch.float64
        if params is None:
            Ws, bs = [W.to(dev, f64) for W in self.W], [b.to(dev, f64) for b in self.b]
        else:
            params = torch.as_tensor(params).detach().to(dev, f64).reshape(P, -1)
            Ws, bs, n_in, at = [], [], F, 0
            for w in self.widths:
                Ws.append(params[:, at:at + w * n_in].reshape(P, w, n_in)); at += w * n_in
                bs.append(params[:, at:at + w]); at += w
                n_in = w
        N = K * (n // P)                                                        # samples of one policy
        x = feat_rows.detach().to(f64).reshape(K, F, P, n // P).permute(2, 1, 0, 3).reshape(P, F, N)
        xs, min_pre = [], float("inf")
        for k, (W, b) in enumerate(zip(Ws, bs)):
            xs.append(x)
            x = torch.matmul(W, x) + b.unsqueeze(2)
            if k + 1 < len(Ws):
                min_pre = min(min_pre, float(x.abs().min()))
                x = torch.tanh(x) if self.hidden == "tanh" else torch.relu(x)
        d = coef.detach().to(f64).reshape(K, P, n // P).permute(1, 0, 2).reshape(P, 1, N)
        grads, scales = [None] * len(Ws), [None] * len(Ws)
        for k in range(len(Ws) - 1, -1, -1):
            grads[k] = torch.cat([torch.matmul(d, xs[k].transpose(1, 2)).reshape(P, -1), d.sum(2)], dim=1)
            scales[k] = torch.cat([torch.matmul(d.abs(), xs[k].abs().transpose(1, 2)).reshape(P, -1), d.abs().sum(2)], dim=1)
            if k:
                a = xs[k]
                d = torch.matmul(Ws[k].transpose(1, 2), d) * ((1.0 - a * a) if self.hidden == "tanh" else (a > 0).to(f64))
        grad = torch.cat(grads, dim=1).contiguous()
        if info:
            return grad, {"scale": torch.cat(scales, dim=1).contiguous(), "min_abs_pre": min_pre}
        return grad

    @staticmethod
    def log_prob(eps, sigma):
        """Log-density of the pre-output sample z = y + sigma eps that collect_mlp acted on, under N(y, sigma^2):
        -eps^2 / 2 - log sigma - log(2 pi) / 2 per env and step.  eps: the "eps" trace [..., n]; sigma: a float, or a tensor
        that broadcasts against eps (one value per env: sigma_per_policy.repeat_interleave(n // P)).  Plain torch,
        differentiable in sigma.  For the likelihood of an old sample under a new network y' and sigma' pass
        eps' = (z - y') / sigma' with y' = the new network's pre-output value on the recorded features (see the example in
        BatchedT1DSimEnv.collect_mlp)."""
        eps = torch.as_tensor(eps)
        sigma = torch.as_tensor(sigma, dtype=eps.dtype, device=eps.device)
        return -0.5 * eps * eps - torch.log(sigma) - 0.5 * math.log(2.0 * math.pi)

    # ------------------------------------------------------------------ the reference's controller surface, one env
    def reset(self):
        self._cgm = None                   # [H, 1] windows, created from the first observation
        self._ins = None
        self._last_basal = 0.0

    def policy(self, observation, reward, done, **info):
        """One env, as SimObj calls it.  The CGM window starts filled with the first observation.  INS uses
        info['insulin'] where the env reports it (the batched env does), else this controller's own last command;
        the time of day comes from info['time'] (a datetime) if present.  With meal_bolus the bolus is that controller's,
        from info['patient_name'], info['meal'] and info['sample_time'] as SimObj passes them.  With relative_to="basal" the
        output multiplies the basal rate BBController gives for info['patient_name']."""
        if self.n_policies != 1:
            raise ValueError("policy() drives one env: it needs a controller with one weight set")
        cgm = torch.tensor([float(observation.CGM)], dtype=torch.float64)
        if self._cgm is None:
            self._cgm = cgm.repeat(self.history, 1)
            self._ins = torch.zeros(self.history, 1, dtype=torch.float64)
        else:
            self.shift(self._cgm, self._ins, cgm, float(info.get("insulin", self._last_basal)))
        now = info.get("time")
        minute = 0 if now is None else now.hour * 60 + now.minute
        meal = torch.tensor([float(info.get("meal", 0.0))], dtype=torch.float64)
        feat = self.features(self._cgm, self._ins, meal, torch.tensor([minute]))
        ref = None
        if self.relative_to is not None:
            bb = self.meal_bolus if self.meal_bolus is not None else BBController()
            ref = torch.tensor([bb._bb_policy(info.get("patient_name"), 0.0, 0.0, 1).basal], dtype=torch.float64)
        self._last_basal = float(self.forward(feat, ordered=True, ref=ref)[0])
        if self.meal_bolus is None:
            return Action(basal=self._last_basal, bolus=0)
        bb = self.meal_bolus._bb_policy(info.get("patient_name"), info.get("meal", 0.0), observation.CGM, info.get("sample_time", 1))
        return Action(basal=self._last_basal, bolus=bb.bolus)
