"""Drop-in ``Flexible_Model`` for the IWAE train-step / NLL hot path.

Mirrors the public surface of the reference class
``flexible_IWAE.Flexible_Model`` (/root/reference/flexible_IWAE.py, "F:"):
same constructor knobs (F:178-F:180), same method names, argument meaning and
return values -- but every number is computed by the HIP library
(libiwae_hip.so, gfx950) through the C ABI of include/iwae.h.  PyTorch is used
only for device memory, the HIP stream and torch.distributed; there is no CPU
fallback (the constructor raises without a GPU or without the library).

Differences a user of the reference should know about (all deliberate):
  * ``train_step`` returns ``{loss_function: float}``; ``fit`` runs the
    Keras-style epoch/batch loop over a device-resident copy of the data.
  * ``dataset_bias`` may be a 784-vector of training pixel means (the quantity
    F:170-F:175 derives from the downloaded dataset) or ``None``; dataset
    names need the mean stored locally (no network): ``$IWAE_DATA_DIR/
    {mnist,omniglot}_train_mean.npy``.
  * Every evaluation entry point accepts an optional ``eps=`` list of
    ``[k, B, d_i]`` noise arrays (the reference's sample-major layout) so runs
    can be reproduced exactly; by default noise is drawn on device (Philox).
  * ``loss_function`` additionally accepts "MIWAE" and "PIWAE" (k = k1*k2,
    IWAE_replication.pdf p7); an unknown name raises ValueError where the
    reference hits UnboundLocalError (F:242).
  * ``loss_function`` also accepts "IWAE_STL" (Roeder et al. 2017) and
    "IWAE_DREG" (Tucker et al. 2019): the IWAE loss value and decoder gradient,
    the encoder's gradient taken through the sampling path only (weights
    softmax / softmax squared).  They run on the fused row-block or layer-wise
    kernels (``kernel_path`` "auto", "fused", "layerwise"), not on the engine.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib

LOSSES = tuple(_lib.LOSS_IDS)


# ----------------------------------------------------------------- helpers
def architecture(n_hidden_encoder, n_hidden_decoder, n_latent_encoder, n_latent_decoder, x_dim=784):
    """Validate the constructor knobs and return the Dense layers in Keras
    ``trainable_weights`` order as (name, fan_in, fan_out) (F:22-F:96)."""
    he, hd = [int(v) for v in n_hidden_encoder], [int(v) for v in n_hidden_decoder]
    le, ld = [int(v) for v in n_latent_encoder], [int(v) for v in n_latent_decoder]
    L = len(he)
    if L < 1 or L > _lib.MAX_LAYERS:
        raise ValueError(f"need 1..{_lib.MAX_LAYERS} stochastic layers")
    if len(le) != L or len(hd) != L or len(ld) != L:
        raise ValueError("n_hidden_encoder, n_hidden_decoder, n_latent_encoder and n_latent_decoder "
                         "must have one entry per stochastic layer (F:206-F:209)")
    if min(he + hd + le) <= 0:
        raise ValueError("layer sizes must be positive")
    for i in range(L - 1):
        if ld[i] != le[L - 2 - i]:
            raise ValueError(f"n_latent_decoder[{i}]={ld[i]} must equal n_latent_encoder[{L-2-i}]={le[L-2-i]} "
                             "(decoder layer i models h_{L-1-i}, F:139-F:140)")
    dense = []
    for i in range(L):
        fin = x_dim if i == 0 else le[i - 1]
        dense += [(f"enc{i}.l1", fin, he[i]), (f"enc{i}.l2", he[i], he[i]),
                  (f"enc{i}.lmu", he[i], le[i]), (f"enc{i}.lstd", he[i], le[i])]
    for i in range(L - 1):
        fin = le[L - 1 - i]
        dense += [(f"dec{i}.l1", fin, hd[i]), (f"dec{i}.l2", hd[i], hd[i]),
                  (f"dec{i}.lmu", hd[i], ld[i]), (f"dec{i}.lstd", hd[i], ld[i])]
    dense += [("out.l1", le[0], hd[-1]), ("out.l2", hd[-1], hd[-1]), ("out.l3", hd[-1], x_dim)]
    return dense


def weight_shapes(dense):
    out = []
    for _, fin, fout in dense:
        out += [(fin, fout), (fout,)]
    return out


def output_bias(train_mean):
    """F:170-F:175: -log(1/clip(mean, .001, .999) - 1)."""
    m = np.clip(np.asarray(train_mean, dtype=np.float64).reshape(-1), 0.001, 0.999)
    return -np.log(1.0 / m - 1.0)


def resolve_dataset_bias(dataset_bias, x_dim=784):
    """Decoder output-bias initialiser (Decoder.get_bias, F:147-F:175)."""
    if dataset_bias is None:
        return np.zeros(x_dim)
    if isinstance(dataset_bias, str):
        name = dataset_bias.lower()
        if "mnist" in name:           # covers F:148 (binarized_mnist) and F:157 (mnist)
            key = "mnist"
        elif "omniglot" in name:      # F:162
            key = "omniglot"
        else:                         # F:167
            raise Exception("Trying to set the initialisation for the bias, "
                            "but the dataset is not recognized")
        d = os.environ.get("IWAE_DATA_DIR")
        path = os.path.join(d, f"{key}_train_mean.npy") if d else None
        if not path or not os.path.exists(path):
            raise FileNotFoundError(
                f"dataset_bias={dataset_bias!r} needs the training pixel means offline: put "
                f"{key}_train_mean.npy (784 values in [0,1]) in $IWAE_DATA_DIR, or pass the mean "
                "vector itself (or None) as dataset_bias")
        return output_bias(np.load(path, allow_pickle=False))
    arr = np.asarray(dataset_bias, dtype=np.float64).reshape(-1)
    if arr.size != x_dim:
        raise ValueError(f"dataset_bias vector must have {x_dim} entries")
    return output_bias(arr)


def glorot_weights(dense, rng, out_bias):
    """Keras defaults: glorot_uniform kernels, zero biases (PDF p8 s3.4)."""
    ws = []
    for name, fin, fout in dense:
        lim = math.sqrt(6.0 / (fin + fout))
        ws.append(rng.uniform(-lim, lim, size=(fin, fout)).astype(np.float32))
        b = np.zeros(fout, np.float32)
        if name == "out.l3":
            b = np.asarray(out_bias, np.float32).reshape(fout)
        ws.append(b)
    return ws


def loss_config(loss_function, k, p=1.0, alpha=1.0, beta=0.5, k1=None, k2=None):
    if loss_function not in _lib.LOSS_IDS:
        raise ValueError(f"unknown loss_function {loss_function!r}; expected one of {LOSSES}")
    if loss_function in ("MIWAE", "PIWAE"):
        if k1 is None or k2 is None:
            raise ValueError(f"{loss_function} needs k1 and k2 (k = k1*k2)")
        k = int(k1) * int(k2)
    return _lib.IwaeLossConfig(_lib.LOSS_IDS[loss_function], int(k), float(p), float(alpha), float(beta),
                               int(k1 or 0), int(k2 or 0))


def ais_schedule(n_temps, kind="sigmoid", rad=4.0):
    """The T + 1 inverse temperatures of an AIS run of T = ``n_temps`` transitions,
    float32, from exactly 0 to exactly 1 and non-decreasing.  ``"linear"``: t / T;
    ``"sigmoid"``: (s(rad (2 t / T - 1)) - s(-rad)) / (s(rad) - s(-rad)) with s the
    logistic function (Wu et al. 2017): small steps where the weights move most."""
    T = int(n_temps)
    if T < 1:
        raise ValueError("n_temps must be at least 1")
    t = np.linspace(0.0, 1.0, T + 1)
    if kind == "linear":
        b = t
    elif kind == "sigmoid":
        s = lambda v: 1.0 / (1.0 + np.exp(-v))
        b = (s(float(rad) * (2.0 * t - 1.0)) - s(-float(rad))) / (s(float(rad)) - s(-float(rad)))
    else:
        raise ValueError('kind must be "linear" or "sigmoid"')
    b = np.maximum.accumulate(np.clip(b, 0.0, 1.0)).astype(np.float32)
    b[0], b[-1] = 0.0, 1.0
    return b


def tvo_schedule(n_part, beta1=0.025):
    """The J + 1 temperatures of a TVO partition of J = ``n_part`` intervals,
    float32: beta_0 = 0, then beta_1 .. beta_J log-uniform from ``beta1`` to
    exactly 1 (Masrani, Le & Wood 2019, section 6).  J = 1 gives [0, 1]."""
    J = int(n_part)
    if J < 1 or J > 64:
        raise ValueError("n_part must be in [1, 64]")
    if J > 1 and not 0.0 < float(beta1) < 1.0:
        raise ValueError("beta1 must lie strictly between 0 and 1")
    b = np.zeros(J + 1, dtype=np.float32)
    b[1:] = np.logspace(np.log10(float(beta1)), 0.0, J) if J > 1 else 1.0
    b[-1] = 1.0
    return b


TVO_OUTPUTS = ("lower", "upper", "iwae", "a_theta", "a_phi")


# --------------------------------------------------------------- optimizer
AGGREGATE_OUTPUTS = ("log_q_agg", "log_q_dim", "log_q_own", "log_q_own_dim", "loc", "scale")


def check_aggregate_args(h1_shape, d1, have_x_ref, components, M, own_period, want):
    """``log_q_aggregate``'s argument rules, on shapes alone: ``h1_shape`` [R, d1]
    or [k, N, d1]; ``components``: the shapes of the loc / scale given (both, each
    [M, d1], or neither); exactly one of x_ref and (loc, scale); 0 <= own_period
    <= M, the own outputs only with own_period > 0.  Returns (R, want)."""
    want = (want,) if isinstance(want, str) else tuple(want)
    bad = [w for w in want if w not in AGGREGATE_OUTPUTS]
    if bad or not [w for w in want if w not in ("loc", "scale")]:
        raise ValueError(f"want must name some of {AGGREGATE_OUTPUTS[:4]} (and may add 'loc', 'scale'), got {want}")
    if len(h1_shape) not in (2, 3) or h1_shape[-1] != d1:
        raise ValueError(f"h1 must be [R, d1={d1}] or [k, N, d1={d1}], got {tuple(h1_shape)}")
    R = int(np.prod(h1_shape[:-1]))
    if R < 1:
        raise ValueError("h1 has no rows")
    if have_x_ref == bool(components):
        raise ValueError("give exactly one of x_ref and (loc, scale)")
    if not have_x_ref and (len(components) != 2 or any(tuple(c) != (M, d1) for c in components)):
        raise ValueError(f"loc and scale must both be given, [M, d1={d1}] each, got {components}")
    if M < 1:
        raise ValueError("no reference components")
    if own_period < 0 or own_period > M:
        raise ValueError(f"own_period must be in [0, M={M}], got {own_period}")
    if own_period == 0 and ("log_q_own" in want or "log_q_own_dim" in want):
        raise ValueError("log_q_own / log_q_own_dim need own_period > 0")
    return R, want


def aggregate_split(R, M, d1):
    """(segments of the joint kernel, segments of the per-unit kernel) into which
    iwae_aggregate splits M references for R query rows of d1 units: the rule
    include/iwae.h documents, restated."""
    def split(wgs, tile):
        n = 1 if wgs >= 1024 else -(-1024 // wgs)
        tiles = -(-M // tile)
        n = min(n, tiles, 1024)
        per = -(-tiles // n)
        return -(-tiles // per)
    uw = min(d1, 256)
    dim_wgs = -(-(-(-R // 4) * uw) // 256) * -(-d1 // uw)
    return split(-(-R // 64), 64), split(dim_wgs, min(128, 4096 // uw))


class Adam:
    """Keras ``tf.keras.optimizers.Adam`` knobs used by E:36-E:40 (defaults are
    Keras' own).  Setting ``learning_rate`` (E:76) updates every compiled model."""

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7):
        self._lr = float(learning_rate)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self._models = []

    @property
    def learning_rate(self):
        return self._lr

    @learning_rate.setter
    def learning_rate(self, v):
        self._lr = float(v)
        for m in self._models:
            m._push_adam()

    lr = learning_rate


# ------------------------------------------------------------------ model
class _Decoder:
    """``model.decoder``: the reference's ``mdl.decoder.generate_x(h)``
    (F:107-F:119) forwarded to the model (held weakly: no reference cycle)."""

    def __init__(self, model):
        import weakref
        self._model = weakref.ref(model)

    def generate_x(self, h, eps=None):
        return self._model().generate_x(h, eps=eps)

    def __call__(self, h):
        """Decoder.call (F:100-F:105): (probs, pxIh) of the given latents, probs
        [n, B, x_dim]; pxIh carries ``.probs`` (the Bernoulli's parameter)."""
        probs = self._model().score(None, h, want=("probs",))["probs"]
        return probs, _Bernoulli(probs)

    def get_log_pxIh(self, x, h):
        """F:123-F:129: log p(x | h_1), [n, B]."""
        return self._model().score(x, h, want=("log_px",))["log_px"]

    def get_log_ph(self, h):
        """F:131-F:142: log p(h), [n, B]."""
        return self._model().score(None, h, want=("log_ph",))["log_ph"]

    def get_log_pxh(self, x, h):
        """F:144-F:145: log p(x, h) = log p(x | h_1) + log p(h), [n, B]."""
        out = self._model().score(x, h, want=("log_ph", "log_px"))
        return out["log_px"] + out["log_ph"]


class _Bernoulli:
    """The thin stand-in for the reference's ``pxIh`` (F:104): its ``probs``."""

    def __init__(self, probs):
        self.probs = probs


class _Normal:
    """The thin stand-in for the reference's ``q_top`` (F:75): ``loc`` and ``scale``."""

    def __init__(self, loc, scale):
        self.loc, self.scale = loc, scale


class _Encoder:
    """``model.encoder``: the reference's ``mdl.encoder(x, n_samples)`` (F:56-F:75)
    forwarded to the model (held weakly: no reference cycle)."""

    def __init__(self, model):
        import weakref
        self._model = weakref.ref(model)
        self.n_stochastic = len(model.n_hidden_encoder)

    def __call__(self, x, n_samples, eps=None, chunk=0):
        """(h, log_qhIx, q_top): h a list of [n_samples, B, d_i] device tensors,
        log_qhIx [n_samples, B], q_top with ``.loc`` / ``.scale`` ([B, d_1] when
        L = 1, [n_samples, B, d_L] otherwise).  ``eps``: L arrays [n_samples, B,
        d_i] (default: device noise, which advances the noise position)."""
        return self._model()._encode(x, n_samples, eps, chunk)


class Flexible_Model:
    """HIP-backed ``Flexible_Model`` (F:177-F:545)."""

    def __init__(self, n_hidden_encoder, n_hidden_decoder, n_latent_encoder, n_latent_decoder,
                 dataset_bias="Binarized_MNIST", loss_function="VAE", k=50, p=1, alpha=1, beta=0.5,
                 *, k1=None, k2=None, x_dim=784, device=None, seed=None, use_graphs=True,
                 kernel_path="auto", precision="bf16x3", tuning=None, **kwargs):
        self.dense = architecture(n_hidden_encoder, n_hidden_decoder, n_latent_encoder, n_latent_decoder, x_dim)
        loss_config(loss_function, k, p, alpha, beta, k1, k2)   # validate early
        if not torch.cuda.is_available():
            raise RuntimeError("Flexible_Model runs on the HIP library only and needs a ROCm GPU "
                               "(no CPU fallback)")
        self._lib = _lib.load()
        self.n_hidden_encoder = list(n_hidden_encoder)
        self.n_hidden_decoder = list(n_hidden_decoder)
        self.n_latent_encoder = list(n_latent_encoder)
        self.n_latent_decoder = list(n_latent_decoder)
        self.n_stochastic_encoder = len(n_hidden_encoder)      # F:210
        self.n_stochastic_decoder = len(n_hidden_decoder)      # F:211
        self.dataset_bias = dataset_bias
        self.loss_function = loss_function
        self.k, self.p, self.alpha, self.beta = k, p, alpha, beta
        self.k1, self.k2 = k1, k2
        self.x_dim = x_dim
        self.epoch = 0                                          # F:218
        self.optimizer = None
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        self._dp = None
        cfg = _lib.IwaeConfig()
        L = len(self.n_hidden_encoder)
        cfg.n_stochastic = L
        cfg.x_dim = x_dim
        for i in range(L):
            cfg.n_hidden_encoder[i] = self.n_hidden_encoder[i]
            cfg.n_latent_encoder[i] = self.n_latent_encoder[i]
            cfg.n_hidden_decoder[i] = self.n_hidden_decoder[i]
            cfg.n_latent_decoder[i] = self.n_latent_decoder[i]
        h = self._lib.iwae_create(cfg, self.device.index)
        if not h:
            raise RuntimeError(f"iwae_create failed: {self._lib.iwae_create_error().decode()}")
        self._h = h
        self._stream = torch.cuda.Stream(device=self.device)
        self._call(self._lib.iwae_set_stream(h, ctypes_stream(self._stream)))
        self._nparams = int(self._lib.iwae_num_params(h))
        if seed is None:
            seed = int.from_bytes(os.urandom(8), "little")
        self._call(self._lib.iwae_set_seed(h, int(seed) & ((1 << 64) - 1)))
        self._seed, self._hmc_gen = int(seed) & ((1 << 64) - 1), None
        self._call(self._lib.iwae_set_graphs(h, 1 if use_graphs else 0))
        paths = {"auto": 0, "layerwise": 1, "fused": 2, "engine": 3}
        if kernel_path not in paths:
            raise ValueError(f"kernel_path must be one of {tuple(paths)}")
        self._call(self._lib.iwae_set_path(h, paths[kernel_path]))
        precisions = {"f32": 0, "bf16x3": 1}
        if precision not in precisions:
            raise ValueError(f"precision must be one of {tuple(precisions)}")
        self._call(self._lib.iwae_set_precision(h, precisions[precision]))
        for name, value in (tuning or {}).items():
            self.set_tuning(name, value)
        rng = np.random.default_rng(int(seed) & ((1 << 63) - 1))
        self.set_weights(glorot_weights(self.dense, rng, resolve_dataset_bias(dataset_bias, x_dim)))
        self._loss_buf = torch.zeros(1, device=self.device)
        self._scratch = torch.zeros(1, device=self.device)
        self.decoder = _Decoder(self)                         # mdl.decoder(h), .generate_x(h), .get_log_*; F:100-F:145
        self.encoder = _Encoder(self)                         # mdl.encoder(x, n_samples), F:56-F:75

    # ------------------------------------------------------------- plumbing
    def set_seed(self, seed):
        """Re-key the device Philox stream and restart its counter (reproducible
        draws from here on).  The reference has no seed."""
        self._call(self._lib.iwae_set_seed(self._h, int(seed) & ((1 << 64) - 1)))
        self._seed, self._hmc_gen = int(seed) & ((1 << 64) - 1), None

    def set_noise_stream(self, stream):
        """Select the noise stream (one per rank: Philox key derived from (seed,
        stream); stream 0 is the seed's own).  Each stream continues from its
        own counter position (re-selecting the current stream is a no-op);
        ``set_seed`` restarts them all."""
        self._call(self._lib.iwae_set_noise_stream(self._h, int(stream) & ((1 << 64) - 1)))

    def set_tuning(self, name, value):
        """Kernel-variant / tuning knob of the library (include/iwae.h enum
        iwae_knob, e.g. ``set_tuning("upd", 0)``): for A/B measurements and the
        variant-agreement tests; the defaults are the measured-fastest paths."""
        if name == "st_wt":      # the store-policy mask has its own entry point (iwae_set_store_policy)
            self._call(self._lib.iwae_set_store_policy(self._h, int(value)))
            return
        if name not in _lib.KNOBS:
            raise ValueError(f"unknown tuning knob {name!r}; expected one of {tuple(_lib.KNOBS)}")
        self._call(self._lib.iwae_set_tuning(self._h, _lib.KNOBS[name], int(value)))

    def _call(self, rc):
        _lib.check(self._lib, self._h, rc)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.iwae_destroy(h)
            except Exception:
                pass
            self._h = None

    def _x(self, x):
        t = torch.as_tensor(x)
        if t.dim() < 2:
            raise ValueError("x must be [B, 28, 28, 1] or [B, 784]")
        t = t.reshape(t.shape[0], int(np.prod(t.shape[1:])))     # explicit width: an empty batch stays [0, 784]
        if t.shape[1] != self.x_dim:                      # F:57 assert(x.shape[1] == 28*28)
            raise ValueError(f"x must flatten to {self.x_dim} pixels, got {t.shape[1]}")
        with torch.cuda.stream(self._stream):
            return t.to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()

    def _mask(self, mask, N):
        """A pixel mask as a device [N, x_dim] float tensor (non-zero = observed)."""
        with torch.cuda.stream(self._stream):
            mt = torch.as_tensor(mask).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
        if mt.dim() < 2 or mt.shape[0] != N or mt.numel() != N * self.x_dim:
            raise ValueError(f"mask must be [N={N}, {self.x_dim}], got {tuple(mt.shape)}")
        return mt.reshape(N, self.x_dim)

    def _eps(self, eps, B, k, n_draws=1):
        if eps is None:
            return None, 0, []
        eps = list(eps)
        L = len(self.n_latent_encoder)
        if len(eps) != n_draws * L:
            raise ValueError(f"expected {n_draws * L} eps arrays, got {len(eps)}")
        ts = []
        with torch.cuda.stream(self._stream):
            for i, e in enumerate(eps):
                t = torch.as_tensor(e).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
                d = self.n_latent_encoder[i % L]
                if tuple(t.shape) != (k, B, d):
                    raise ValueError(f"eps[{i}] must be [k={k}, B={B}, d={d}], got {tuple(t.shape)}")
                ts.append(t)
        arr, n = _lib.fptr_array(ts)
        return arr, n, ts

    def _scalar(self, fn, *args):
        with torch.cuda.stream(self._stream):
            out = torch.empty(1, device=self.device)
        self._call(fn(self._h, *args, _lib.fptr(out)))
        self._stream.synchronize()
        return float(out.item())

    def _lc(self, loss_function=None, k=None, p=None, alpha=None, beta=None, k1=None, k2=None):
        return loss_config(loss_function or self.loss_function, self.k if k is None else k,
                           self.p if p is None else p, self.alpha if alpha is None else alpha,
                           self.beta if beta is None else beta,
                           self.k1 if k1 is None else k1, self.k2 if k2 is None else k2)

    # ------------------------------------------------------------- weights
    @property
    def trainable_weights(self):
        return self.get_weights()

    def get_weights(self):
        flat = np.empty(self._nparams, np.float32)
        self._call(self._lib.iwae_get_params(self._h, flat.ctypes.data_as(_lib.FP), flat.size))
        return _split(flat, weight_shapes(self.dense))

    def set_weights(self, weights):
        flat = _join(weights, weight_shapes(self.dense))
        self._call(self._lib.iwae_set_params(self._h, flat.ctypes.data_as(_lib.FP), flat.size))

    def get_gradients(self):
        """Gradient of the loss from the last train step / forward_backward."""
        flat = np.empty(self._nparams, np.float32)
        self._call(self._lib.iwae_get_grads(self._h, flat.ctypes.data_as(_lib.FP), flat.size))
        return _split(flat, weight_shapes(self.dense))

    def get_optimizer_state(self):
        m = np.empty(self._nparams, np.float32)
        v = np.empty(self._nparams, np.float32)
        import ctypes
        step = ctypes.c_longlong(0)
        self._call(self._lib.iwae_get_adam_state(self._h, m.ctypes.data_as(_lib.FP), v.ctypes.data_as(_lib.FP),
                                                 m.size, ctypes.byref(step)))
        return m, v, int(step.value)

    def set_optimizer_state(self, m, v, step):
        m = np.ascontiguousarray(m, np.float32)
        v = np.ascontiguousarray(v, np.float32)
        self._call(self._lib.iwae_set_adam_state(self._h, m.ctypes.data_as(_lib.FP), v.ctypes.data_as(_lib.FP),
                                                 m.size, int(step)))

    def save_weights(self, path):
        """Weights + Adam state as .npz (the reference uses TF checkpoints, E:95)."""
        m, v, step = self.get_optimizer_state()
        ws = self.get_weights()
        np.savez(path, *ws, adam_m=m, adam_v=v, adam_step=np.int64(step), epoch=np.int64(self.epoch))

    def load_weights(self, path):
        with np.load(path, allow_pickle=False) as z:
            n = len(weight_shapes(self.dense))
            self.set_weights([z[f"arr_{i}"] for i in range(n)])
            if "adam_m" in z:
                self.set_optimizer_state(z["adam_m"], z["adam_v"], int(z["adam_step"]))
            if "epoch" in z:
                self.epoch = int(z["epoch"])

    # ------------------------------------------------------------- training
    def compile(self, optimizer=None, **kwargs):
        self.optimizer = optimizer if optimizer is not None else Adam()
        if self not in self.optimizer._models:
            self.optimizer._models.append(self)
        self._push_adam()

    def _push_adam(self):
        o = self.optimizer
        self._call(self._lib.iwae_set_adam(self._h, o.learning_rate, o.beta_1, o.beta_2, o.epsilon))

    def train_step(self, x, eps=None, sync=True, mask=None):
        """F:221-F:247: one optimisation step; returns {loss_function: loss}.
        ``x`` [B, x_dim]: pixels in [0, 1].  Images of 0s and 1s take the
        one-log form of the Bernoulli log-probability, grey levels the two-log
        form x log p + (1 - x) log(1 - p) (F:127-F:128) -- the same function,
        decided per tile of sample rows or per workgroup, so a binarised image
        may take either form depending on its neighbours in the batch (equal
        to float32 rounding, not bit for bit).
        ``mask`` [B, x_dim] (non-zero = observed): the step on incomplete images
        (iwae_train_step_masked; Mattei & Frellsen 2019): the encoder sees
        x * mask, the likelihood sums the observed pixels, whatever ``x`` holds
        at a missing pixel is ignored (NaN included)."""
        if self.optimizer is None:
            self.compile()
        xd = self._x(x)
        B = xd.shape[0]
        lc = self._lc()
        arr, n, keep = self._eps(eps, B, lc.k, 2 if self.loss_function == "CIWAE" else 1)
        if mask is not None:
            if self._dp is not None:
                raise ValueError("train_step(mask=...) is not supported under data parallelism")
            mt = self._mask(mask, B)
            self._call(self._lib.iwae_train_step_masked(self._h, lc, _lib.fptr(xd), _lib.fptr(mt), B, arr, n,
                                                        _lib.fptr(self._loss_buf)))
        elif self._dp is not None:
            self._dp.step(self, lc, xd, B, arr, n)
        else:
            self._call(self._lib.iwae_train_step(self._h, lc, _lib.fptr(xd), B, arr, n, _lib.fptr(self._loss_buf)))
        self.epoch += 1                                                   # F:245
        if not sync:
            return {self.loss_function: self._loss_buf}
        self._stream.synchronize()
        loss = float(self._loss_buf.item())
        self._call(self._lib.iwae_status(self._h))      # an in-launch wait that gave up raises
        return {self.loss_function: loss}

    def train_steps(self, x, batch_size, sync=True, mask=None):
        """len(x) // batch_size consecutive train steps (F:221-F:247 each) on the
        batches x[i*batch_size:(i+1)*batch_size] with device noise: fit's inner
        loop (E:82) as one library call (iwae_train_steps: up to 32 steps per
        captured graph).  Returns the per-step losses (device tensor if
        sync=False).  ``mask`` [len(x), x_dim]: pixel-masked steps (see
        train_step), one iwae_train_step_masked per batch on the stream with no
        synchronisation between them."""
        if self.optimizer is None:
            self.compile()
        xd = self._x(x)
        B = int(batch_size)
        if B <= 0:
            raise ValueError("batch_size must be positive")
        n = xd.shape[0] // B
        with torch.cuda.stream(self._stream):
            losses = torch.empty(n, device=self.device)
        if n == 0:
            return losses if not sync else losses.cpu().numpy()
        if mask is not None:
            if self._dp is not None:
                raise ValueError("train_steps(mask=...) is not supported under data parallelism")
            mt = self._mask(mask, xd.shape[0])
            lc = self._lc()
            for i in range(n):
                self._call(self._lib.iwae_train_step_masked(
                    self._h, lc, _lib.fptr(xd[i * B:(i + 1) * B]), _lib.fptr(mt[i * B:(i + 1) * B]), B, None, 0,
                    _lib.fptr(self._loss_buf)))
                with torch.cuda.stream(self._stream):
                    losses[i] = self._loss_buf[0]
        elif self._dp is not None and self._dp.comm != "library":
            for i in range(n):
                self._dp.step(self, self._lc(), xd[i * B:(i + 1) * B], B, None, 0)
                with torch.cuda.stream(self._stream):
                    losses[i] = self._loss_buf[0]
        else:
            self._call(self._lib.iwae_train_steps(self._h, self._lc(), _lib.fptr(xd), B, n, _lib.fptr(losses)))
        self.epoch += n                                                   # F:245, per step
        if not sync:
            return losses
        self._stream.synchronize()
        out = losses.cpu().numpy()
        self._call(self._lib.iwae_status(self._h))      # an in-launch wait that gave up raises
        return out

    def prepare_train_steps(self, x, batch_size):
        """Capture every graph train_steps(x, batch_size) will replay, without
        running a step (iwae_train_steps_prepare): a timed loop then measures
        replays only.  Parameters, Adam state and noise are untouched."""
        if self.optimizer is None:
            self.compile()
        xd = self._x(x)
        B = int(batch_size)
        if B <= 0:
            raise ValueError("batch_size must be positive")
        n = xd.shape[0] // B
        if n and not (self._dp is not None and self._dp.comm != "library"):
            self._call(self._lib.iwae_train_steps_prepare(self._h, self._lc(), _lib.fptr(xd), B, n))

    # ----------------------------------------------------- reweighted wake-sleep
    def _dreams(self, dreams):
        """(x_dream, [h_1 .. h_L]) as contiguous device tensors [n, x_dim] and
        [n, d_i]; (x tensor, latent tensors, n)."""
        try:
            xs, hs = dreams
            hs = list(hs)
        except (TypeError, ValueError):
            raise ValueError("dreams must be (x_dream, [h_1 .. h_L])") from None
        dims = self.n_latent_encoder
        if len(hs) != len(dims):
            raise ValueError(f"expected {len(dims)} dream latent arrays (one per stochastic layer), got {len(hs)}")
        xt = self._x(xs)
        n = int(xt.shape[0])
        ts = []
        with torch.cuda.stream(self._stream):
            for i, v in enumerate(hs):
                t = torch.as_tensor(v).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
                if tuple(t.shape) != (n, dims[i]):
                    raise ValueError(f"dream h[{i}] must be [n={n}, d={dims[i]}], got {tuple(t.shape)}")
                ts.append(t)
        return xt, ts, n

    def _wake_sleep(self, xd, c_wake, c_sleep, n_dream, dreams, k, eps, update, values):
        """One iwae_wake_sleep_step / _grad on the device batch xd; the three
        values into the device tensor ``values`` (3 floats)."""
        if self._dp is not None:
            raise ValueError("wake_sleep_step is not supported under data parallelism")
        if self.optimizer is None:
            self.compile()
        B = int(xd.shape[0])
        k = self.k if k is None else int(k)
        c_wake, c_sleep = float(c_wake), float(c_sleep)
        dx, dh, harr, nh = None, [], None, 0
        if dreams is not None:
            dx, dh, n = self._dreams(dreams)
            if n_dream is not None and int(n_dream) != n:
                raise ValueError(f"n_dream = {n_dream} but the dreams hold {n} rows")
            harr, nh = _lib.fptr_array(dh)
            if c_sleep == 0.0:
                n = 0                        # the dreams are never read
        elif n_dream is None:
            n = B if c_sleep > 0.0 else 0
        else:
            n = int(n_dream)
        arr, ne, keep = self._eps(eps, B, k)
        cfg = _lib.IwaeWsConfig(k, n, c_wake, c_sleep)
        fn = self._lib.iwae_wake_sleep_step if update else self._lib.iwae_wake_sleep_grad
        self._call(fn(self._h, cfg, _lib.fptr(xd), B, arr, ne, _lib.fptr(dx), harr, nh, _lib.fptr(values)))
        if update:
            self.epoch += 1
        return keep, dx, dh                  # alive until the caller has synchronised or moved on in stream order

    def wake_sleep_step(self, x, c_wake=1.0, c_sleep=0.0, n_dream=None, dreams=None, k=None, eps=None, sync=True,
                        update=True):
        """One reweighted wake-sleep step (iwae_wake_sleep_step; Bornschein &
        Bengio 2015, Le et al. 2019): the decoder takes the IWAE gradient of a
        k-sample wake forward on ``x``; the encoder descends
        c_wake L_wake + c_sleep L_sleep, with L_wake = -mean_b sum_s
        softmax_s(log w) log q(h_bs | x_b) at the wake samples and weights held
        fixed and L_sleep = -mean_j log q(h^j | x^j) over dream pairs.  (1, 0) is
        wake-wake, (0, 1) wake-sleep, (0.5, 0.5) the mix.  ``dreams`` =
        (x_dream [n, x_dim], [h_1 .. h_L] each [n, d_i]), numpy arrays or device
        tensors (any (x, h) pairs: the states ``ais`` or ``hmc`` leave, say);
        without them the step dreams ``n_dream`` pairs (default: the batch size
        when c_sleep > 0) from the current weights, as ``sample`` would.  ``k``
        defaults to the model's; ``eps`` as for ``train_step``.
        ``update=False`` leaves the gradient in the buffer (``get_gradients``)
        and Adam untouched.  Returns {"IWAE": L_theta, "wake": L_wake, "sleep":
        L_sleep} (a phase whose coefficient is 0 reports 0); device scalars
        with ``sync=False``."""
        xd = self._x(x)
        with torch.cuda.stream(self._stream):
            values = torch.empty(3, device=self.device)
        keep = self._wake_sleep(xd, c_wake, c_sleep, n_dream, dreams, k, eps, update, values)
        if not sync:
            self._ws_keep = (xd, keep)
            return {"IWAE": values[0], "wake": values[1], "sleep": values[2]}
        self._stream.synchronize()
        v = values.cpu().numpy()
        self._call(self._lib.iwae_status(self._h))
        return {"IWAE": float(v[0]), "wake": float(v[1]), "sleep": float(v[2])}

    def wake_sleep_steps(self, x, batch_size, c_wake=1.0, c_sleep=0.0, n_dream=None, k=None, sync=True):
        """len(x) // batch_size consecutive wake-sleep steps on the batches
        x[i*batch_size:(i+1)*batch_size] with device noise and the steps' own
        dreams, enqueued without synchronising between them.  Returns the
        values [nsteps, 3] (IWAE, wake, sleep per step; a device tensor with
        sync=False)."""
        xd = self._x(x)
        B = int(batch_size)
        if B <= 0:
            raise ValueError("batch_size must be positive")
        n = xd.shape[0] // B
        with torch.cuda.stream(self._stream):
            values = torch.zeros(n, 3, device=self.device)
        for i in range(n):
            self._wake_sleep(xd[i * B:(i + 1) * B], c_wake, c_sleep, n_dream, None, k, None, True, values[i])
        if not sync:
            self._ws_keep = (xd,)
            return values
        self._stream.synchronize()
        out = values.cpu().numpy()
        self._call(self._lib.iwae_status(self._h))
        return out

    # --------------------------------------- thermodynamic variational objective
    @staticmethod
    def _betas(betas, n_part):
        if betas is None:
            return tvo_schedule(5 if n_part is None else n_part)
        bt = np.ascontiguousarray(betas, dtype=np.float32).ravel()
        if n_part is not None and int(n_part) != bt.size - 1:
            raise ValueError(f"n_part = {n_part} but betas holds {bt.size} values")
        if bt.size < 2:
            raise ValueError("betas must hold at least two values")
        return bt

    def _tvo(self, xd, bt, k, eps, update, values):
        """One iwae_tvo_step / _grad on the device batch xd; the three values
        into the device tensor ``values`` (3 floats)."""
        if self._dp is not None:
            raise ValueError("tvo_step is not supported under data parallelism")
        if self.optimizer is None:
            self.compile()
        B = int(xd.shape[0])
        k = self.k if k is None else int(k)
        arr, ne, keep = self._eps(eps, B, k)
        cfg = _lib.IwaeTvoConfig(k, bt.size - 1)
        fn = self._lib.iwae_tvo_step if update else self._lib.iwae_tvo_grad
        self._call(fn(self._h, cfg, bt.ctypes.data_as(_lib.FP), _lib.fptr(xd), B, arr, ne, _lib.fptr(values)))
        if update:
            self.epoch += 1
        return keep                          # alive until the caller has synchronised or moved on in stream order

    def tvo_step(self, x, betas=None, n_part=None, k=None, eps=None, sync=True, update=True):
        """One step on the thermodynamic variational objective (iwae_tvo_step;
        Masrani, Le & Wood 2019): over the partition ``betas`` (default
        ``tvo_schedule(n_part or 5)``) of [0, 1], the left Riemann sum of
        m(beta) = E_softmax(beta log w)[log w] over a k-sample wake forward on
        ``x``.  The decoder descends it at fixed samples, the encoder takes the
        covariance-form gradient (no reparameterisation).  ``k`` defaults to
        the model's; ``eps`` as for ``train_step``.  ``update=False`` leaves the
        gradient in the buffer (``get_gradients``) and Adam untouched.  Returns
        {"TVO": L_tvo, "TVO_upper": L_upper, "IWAE": L_iwae}, the negated batch
        means of lower <= iwae <= upper (so TVO >= IWAE >= TVO_upper); device
        scalars with ``sync=False``."""
        xd = self._x(x)
        bt = self._betas(betas, n_part)
        with torch.cuda.stream(self._stream):
            values = torch.empty(3, device=self.device)
        keep = self._tvo(xd, bt, k, eps, update, values)
        if not sync:
            self._tvo_keep = (xd, keep)
            return {"TVO": values[0], "TVO_upper": values[1], "IWAE": values[2]}
        self._stream.synchronize()
        v = values.cpu().numpy()
        self._call(self._lib.iwae_status(self._h))
        return {"TVO": float(v[0]), "TVO_upper": float(v[1]), "IWAE": float(v[2])}

    def tvo_steps(self, x, batch_size, betas=None, n_part=None, k=None, sync=True):
        """len(x) // batch_size consecutive TVO steps on the batches
        x[i*batch_size:(i+1)*batch_size] with device noise, enqueued without
        synchronising between them.  Returns the values [nsteps, 3] (TVO,
        TVO_upper, IWAE per step; a device tensor with sync=False)."""
        xd = self._x(x)
        B = int(batch_size)
        if B <= 0:
            raise ValueError("batch_size must be positive")
        bt = self._betas(betas, n_part)
        n = xd.shape[0] // B
        with torch.cuda.stream(self._stream):
            values = torch.zeros(n, 3, device=self.device)
        for i in range(n):
            self._tvo(xd[i * B:(i + 1) * B], bt, k, None, True, values[i])
        if not sync:
            self._tvo_keep = (xd,)
            return values
        self._stream.synchronize()
        out = values.cpu().numpy()
        self._call(self._lib.iwae_status(self._h))
        return out

    def tvo_bounds(self, lw, betas, want=("lower", "upper", "iwae")):
        """iwae_tvo_weights on log weights ``lw`` [N, k] (a numpy array or a
        device tensor, image-major: ``get_log_weights(...).T``, ``ais``' or
        ``refine``'s): per image the TVO sandwich lower <= iwae <= upper over
        the partition ``betas``, and on request the per-sample coefficients
        "a_theta" and "a_phi" [N, k].  Returns a dict of device tensors named
        as in ``want``.  Nothing is drawn and no state changes."""
        want = tuple(want)
        if not want or any(w not in TVO_OUTPUTS for w in want):
            raise ValueError(f"want must name some of {TVO_OUTPUTS}")
        bt = self._betas(betas, None)
        with torch.cuda.stream(self._stream):
            lt = torch.as_tensor(lw).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
            if lt.dim() != 2:
                raise ValueError(f"lw must be [N, k], got {tuple(lt.shape)}")
            N, k = int(lt.shape[0]), int(lt.shape[1])
            out = {w: torch.empty((N, k) if w.startswith("a_") else (N,), device=self.device) for w in want}
        self._call(self._lib.iwae_tvo_weights(self._h, _lib.fptr(lt), N, k, bt.ctypes.data_as(_lib.FP), bt.size - 1,
                                              *[_lib.fptr(out.get(w)) for w in TVO_OUTPUTS]))
        self._stream.synchronize()
        return out

    def get_L_TVO(self, x, k, betas=None, eps=None):
        """The model's k log weights per image through ``tvo_bounds``: the batch
        means (lower, upper, iwae), lower <= iwae <= upper (``betas`` default:
        ``tvo_schedule(5)``)."""
        lw = self.get_log_weights(x, k, eps=eps)
        with torch.cuda.stream(self._stream):
            lw = lw.t().contiguous()
        out = self.tvo_bounds(lw, self._betas(betas, None))
        return tuple(float(out[w].double().mean().item()) for w in ("lower", "upper", "iwae"))

    def graph_captures(self):
        """Train-step graphs captured so far (iwae_debug_count id 7)."""
        return int(self._lib.iwae_debug_count(self._h, 7))

    def check_kernel_status(self):
        """Synchronize and raise if a kernel reported a failure: an in-launch
        wait of the combined image-row backward + update launch that gave up
        (iwae_status; give-ups counted by iwae_debug_count id 8)."""
        self._call(self._lib.iwae_synchronize(self._h))
        n = int(self._lib.iwae_debug_count(self._h, 8))
        if n:
            raise _lib.IwaeError(f"{n} in-launch wait(s) gave up")

    def _binarize(self, x, perm, u, out):
        """binarize without the final synchronize (fit's per-epoch call)."""
        xd = self._x(x)
        n_src, xdim = xd.shape[0], self.x_dim
        pt = None
        if perm is not None:
            with torch.cuda.stream(self._stream):
                pt = torch.as_tensor(perm)
                if pt.dim() != 1 or pt.dtype.is_floating_point or pt.dtype.is_complex or pt.dtype == torch.bool:
                    raise ValueError(f"perm must be a 1-d integer array, got {tuple(pt.shape)} of {pt.dtype}")
                pt = pt.to(device=self.device, dtype=torch.int64).contiguous()
        n = n_src if pt is None else int(pt.shape[0])
        if n > 1 << 24:
            raise ValueError("more than 2^24 output rows per call are not supported")
        ut = None
        if u is not None:
            with torch.cuda.stream(self._stream):
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(ut.shape) != (n, xdim):
                raise ValueError(f"u must be [n={n}, {xdim}], got {tuple(ut.shape)}")
        ld = (xdim + 3) // 4 * 4
        if out is None:
            with torch.cuda.stream(self._stream):
                out = torch.empty(n, ld, device=self.device)[:, :xdim]
        else:
            if (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
                    or tuple(out.shape) != (n, xdim) or (xdim > 1 and out.stride(1) != 1)):
                raise ValueError(f"out must be a float32 tensor [n={n}, {xdim}] on {self.device} with unit column "
                                 "stride")
            if n > 1:
                ld = out.stride(0)
        if n > 0:
            rc = self._lib.iwae_binarize(self._h, _lib.fptr(xd), n_src,
                                         None if pt is None else ctypes.cast(ctypes.c_void_p(pt.data_ptr()),
                                                                             ctypes.POINTER(ctypes.c_longlong)),
                                         n, _lib.fptr(ut), _lib.fptr(out), int(ld))
            if rc != 0:              # the shapes passed above: what is left is a layout the library refuses
                msg = self._lib.iwae_last_error(self._h)
                raise _lib.IwaeError(f"libiwae_hip error {rc}: {msg.decode() if msg else 'unknown error'}")
        return out

    def binarize(self, x, perm=None, u=None, out=None):
        """Dynamic binarisation on the device (iwae_binarize; the stochastic
        "MNIST" setting, PDF p7 s3.1): row i of the result is drawn from the
        grey levels ``x[perm[i]]`` (``perm``: any 1-d integer tensor or array,
        converted to int64 on the device; None: every row of x in order), pixel
        = (u < x or x >= 1) as 0.0 / 1.0 -- Bernoulli(x), with 0/1 images a fixed
        point; an index outside x gives a row of zeros.  One launch, one advance
        of the model's noise position.  Returns a device float32 [n, x_dim]
        tensor on the model's stream.  ``u``: [n, x_dim] uniforms in [0, 1)
        instead of the device's Philox draws (tests).  ``out``: a float32 device
        tensor [n, x_dim] to write into (unit column stride; its row stride is
        the leading dimension: a multiple of 4, its storage 16-byte aligned,
        else IwaeError); ``out=x`` binarises in place when ``perm`` is None."""
        out = self._binarize(x, perm, u, out)
        self._stream.synchronize()
        return out

    def fit(self, x, epochs=1, batch_size=100, shuffle=True, verbose=0, seed=None, mask=None, binarize=False):
        """Keras-style loop (E:82): per epoch shuffle, batches of batch_size
        (last partial batch included), one train step each (the whole batches
        through train_steps, the partial one through train_step).  ``mask``
        [N, x_dim]: training on incomplete images (see train_step); the epoch's
        permutation is applied to x and mask alike.  ``binarize``: x holds grey
        levels and every epoch trains on a fresh dynamic binarisation of it
        (see binarize): one iwae_binarize launch per epoch gathers by the
        epoch's permutation and draws the pixels into a buffer reused across
        epochs, then the epoch's steps follow (noise: one advance for the
        binarisation, then the steps')."""
        xd = self._x(x)
        N = xd.shape[0]
        md = self._mask(mask, N) if mask is not None else None
        g = torch.Generator(device="cpu")
        if seed is not None:
            g.manual_seed(int(seed))
        hist = []
        xb = None
        for ep in range(int(epochs)):
            perm = torch.randperm(N, generator=g) if shuffle else torch.arange(N)
            with torch.cuda.stream(self._stream):
                if binarize:
                    xs = xb = self._binarize(xd, perm if shuffle else None, None, xb)
                else:
                    xs = xd[perm.to(self.device)] if shuffle else xd
                ms = None if md is None else (md[perm.to(self.device)] if shuffle else md)
                losses = torch.zeros((N + batch_size - 1) // batch_size, device=self.device)
            nfull = N // batch_size
            ncut = nfull * batch_size
            if nfull:
                full = self.train_steps(xs[:ncut], batch_size, sync=False, mask=None if ms is None else ms[:ncut])
                with torch.cuda.stream(self._stream):
                    losses[:nfull] = full
            if N % batch_size:
                out = self.train_step(xs[ncut:], sync=False, mask=None if ms is None else ms[ncut:])[self.loss_function]
                with torch.cuda.stream(self._stream):
                    losses[nfull] = out[0]
            self._stream.synchronize()
            hist.append(float(losses.mean().item()))
            if verbose:
                print(f"epoch {ep + 1}/{epochs} - {self.loss_function}: {hist[-1]:.4f}")
        return {self.loss_function: hist}

    # ----------------------------------------------------------- evaluation
    def get_log_weights(self, x, n_samples, eps=None):
        """F:327-F:351: log w, returned sample-major [n_samples, B] like the reference."""
        xd = self._x(x)
        B = xd.shape[0]
        arr, n, keep = self._eps(eps, B, n_samples)
        with torch.cuda.stream(self._stream):
            lw = torch.empty(B, n_samples, device=self.device)
        self._call(self._lib.iwae_log_weights(self._h, _lib.fptr(xd), B, int(n_samples), arr, n, _lib.fptr(lw)))
        with torch.cuda.stream(self._stream):
            out = lw.t().contiguous()
        self._stream.synchronize()
        return out

    @staticmethod
    def L_k_from_weights(log_weights):
        """F:363-F:370 on a [k, B] tensor."""
        lw = torch.as_tensor(log_weights)
        m = lw.max(dim=0).values
        return torch.mean(torch.log(torch.mean(torch.exp(lw - m), dim=0)) + m)

    @staticmethod
    def L_from_weights(log_weights):
        """F:429-F:430."""
        return torch.mean(torch.as_tensor(log_weights))

    def _bound(self, lc, x, eps, n_draws=1, mask=None):
        """A forward-only bound; ``mask`` [B, x_dim] (non-zero = observed): of
        the observed pixels of incomplete images (iwae_bound_masked)."""
        xd = self._x(x)
        B = xd.shape[0]
        arr, n, keep = self._eps(eps, B, lc.k, n_draws)
        if mask is not None:
            mt = self._mask(mask, B)
            return self._scalar(self._lib.iwae_bound_masked, lc, _lib.fptr(xd), _lib.fptr(mt), B, arr, n)
        return self._scalar(self._lib.iwae_bound, lc, _lib.fptr(xd), B, arr, n)

    def get_L_k(self, x, k, eps=None, mask=None):
        """F:354-F:361."""
        return self._bound(self._lc("IWAE", k=k), x, eps, mask=mask)

    def get_L(self, x, k=5000, eps=None, mask=None):
        """F:419-F:427."""
        return self._bound(self._lc("VAE", k=k), x, eps, mask=mask)

    def get_L_median(self, x, k, eps=None, mask=None):
        """F:373-F:379."""
        return self._bound(self._lc("L_median", k=k), x, eps, mask=mask)

    def get_L_CIWAE(self, x, n_samples, beta, eps=None, mask=None):
        """F:382-F:383 (two independent draws: eps = draw1 + draw2)."""
        return self._bound(self._lc("CIWAE", k=n_samples, beta=beta), x, eps, 2, mask=mask)

    def get_L_alpha(self, x, n_samples, alpha, eps=None, mask=None):
        """F:386-F:402."""
        return self._bound(self._lc("L_alpha", k=n_samples, alpha=alpha), x, eps, mask=mask)

    def get_L_power_p(self, x, k, p, eps=None, mask=None):
        """F:405-F:409."""
        return self._bound(self._lc("L_power_p", k=k, p=p), x, eps, mask=mask)

    def get_L_V1(self, x, n_samples, eps=None, mask=None):
        """F:434-F:460."""
        return self._bound(self._lc("VAE_V1", k=n_samples), x, eps, mask=mask)

    def get_L_MIWAE(self, x, k1, k2, eps=None, mask=None):
        """MIWAE(k1, k2) (IWAE_replication.pdf p7)."""
        return self._bound(self._lc("MIWAE", k1=k1, k2=k2), x, eps, mask=mask)

    def get_E_qhIx_log_pxIh(self, x, n_samples, eps=None):
        """F:304-F:325 (Keras binary cross-entropy form)."""
        xd = self._x(x)
        B = xd.shape[0]
        arr, n, keep = self._eps(eps, B, n_samples)
        return self._scalar(self._lib.iwae_e_log_px, _lib.fptr(xd), B, int(n_samples), arr, n)

    def get_Dkl_qhIx_ph(self, x, k):
        """F:414-F:415."""
        return self.get_E_qhIx_log_pxIh(x, k) - self.get_L(x, k)

    def get_Dkl_qhIx_phIx(self, x, k):
        """F:411-F:412."""
        return -1 * (self.get_L(x, k) + self.get_NLL(x))

    def log_px(self, x, k=5000, eps=None, chunk=0):
        """Per-image k-sample log p(x) estimate (device tensor [N]).  ``x``:
        pixels in [0, 1]; 0/1 images take the one-log form of the Bernoulli
        log-probability, grey levels the two-log form (see train_step: decided
        per tile or workgroup, so a binarised image may take either form
        depending on its neighbours)."""
        xd = self._x(x)
        N = xd.shape[0]
        with torch.cuda.stream(self._stream):
            out = torch.empty(N, device=self.device)
        if eps is not None:
            arr, n, keep = self._eps(eps, N, k)
            self._call(self._lib.iwae_nll_eps(self._h, _lib.fptr(xd), N, int(k), arr, n, _lib.fptr(out)))
        else:
            self._call(self._lib.iwae_nll(self._h, _lib.fptr(xd), N, int(k), int(chunk), _lib.fptr(out)))
        self._stream.synchronize()
        return out

    def log_px_partials(self, x, k_local, chunk=0):
        """Per-image log-sum-exp partials over k_local device-noise samples of
        this handle's noise stream: (m, s) with m = max_s lw, s = sum_s exp(lw - m)
        (the sample-sharded NLL's per-rank contribution)."""
        xd = self._x(x)
        N = xd.shape[0]
        with torch.cuda.stream(self._stream):
            m = torch.empty(N, device=self.device)
            s = torch.empty(N, device=self.device)
        self._call(self._lib.iwae_nll_partials(self._h, _lib.fptr(xd), N, int(k_local), int(chunk), _lib.fptr(m),
                                               _lib.fptr(s)))
        self._stream.synchronize()
        return m, s

    def get_NLL(self, x, k=5000, eps=None):
        """F:463-F:464: -L_k with k = 5000 by default."""
        return float(-self.log_px(x, k, eps).mean().item())

    # ------------------------------------------------ evaluation statistics
    def _reconstruct(self, x, eps, want_probs):
        xd = self._x(x)
        B = xd.shape[0]
        L = len(self.n_latent_encoder)
        arr, n, keep = None, 0, []
        if eps is not None:
            eps = list(eps)
            if len(eps) != 2 * L - 1:
                raise ValueError(f"expected {2 * L - 1} eps arrays (encoder, then prior), got {len(eps)}")
            dims = list(self.n_latent_encoder) + [self.n_latent_encoder[L - 2 - j] for j in range(L - 1)]
            with torch.cuda.stream(self._stream):
                for e, d in zip(eps, dims):
                    t = torch.as_tensor(e).to(device=self.device, dtype=torch.float32).contiguous()
                    if tuple(t.shape) != (1, B, d):
                        raise ValueError(f"eps arrays must be [1, B={B}, d={d}], got {tuple(t.shape)}")
                    keep.append(t)
            arr, n = _lib.fptr_array(keep)
        with torch.cuda.stream(self._stream):
            ld = (self.x_dim + 3) // 4 * 4
            probs = torch.empty(B, ld, device=self.device) if want_probs else None
            loss = torch.empty(1, device=self.device)
        self._call(self._lib.iwae_reconstruct(self._h, _lib.fptr(xd), B, arr, n, _lib.fptr(probs),
                                              ld if want_probs else 0, _lib.fptr(loss)))
        self._stream.synchronize()
        return (probs[:, :self.x_dim] if want_probs else None), float(loss.item())

    def reconstructed_x_probs(self, x, eps=None):
        """F:249-F:254: pixel probabilities [1, B, 784] of x reconstructed from
        one q(h|x) draw of h_L through the decoder's prior layers (generate_x,
        F:107-F:119).  ``eps``: L encoder arrays [1,B,d_i], then the L-1 prior
        draws in generation order ([1,B,d_{L-2-j}])."""
        probs, _ = self._reconstruct(x, eps, True)
        return probs.unsqueeze(0)

    def get_reconstruction_loss(self, x, eps=None):
        """F:256-F:262: mean over the batch of the Keras BCE of x against the
        reconstructed probabilities, summed over pixels."""
        return self._reconstruct(x, eps, False)[1]

    # ------------------------------------------------------------ generation
    def _generate(self, n, h_top, eps, u, want_probs, want_pixels, want_latents):
        """iwae_generate on n rows; returns (probs, pixels, latents), each
        None unless asked for.  Arguments are validated before the native call."""
        L = len(self.n_latent_encoder)
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        dims = [] if h_top is not None else [self.n_latent_encoder[L - 1]]
        dims += [self.n_latent_encoder[L - 2 - j] for j in range(L - 1)]
        keep, arr, ne = [], None, 0
        if eps is not None:
            eps = list(eps)
            if len(eps) != len(dims):
                what = "the prior draws" if h_top is not None else "h_L, then the prior draws"
                raise ValueError(f"expected {len(dims)} eps arrays ({what}), got {len(eps)}")
            with torch.cuda.stream(self._stream):
                for e, d in zip(eps, dims):
                    t = torch.as_tensor(e).to(device=self.device, dtype=torch.float32).contiguous()
                    if tuple(t.shape) != (1, n, d):
                        raise ValueError(f"eps arrays must be [1, n={n}, d={d}], got {tuple(t.shape)}")
                    keep.append(t)
            arr, ne = _lib.fptr_array(keep)
        ut = None
        if u is not None:
            with torch.cuda.stream(self._stream):
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(ut.shape) != (n, self.x_dim):
                raise ValueError(f"u must be [n={n}, {self.x_dim}], got {tuple(ut.shape)}")
        with torch.cuda.stream(self._stream):
            ld = (self.x_dim + 3) // 4 * 4
            probs = torch.empty(n, ld, device=self.device) if want_probs else None
            pixels = torch.empty(n, ld, device=self.device) if want_pixels else None
            hs = [torch.empty(n, d, device=self.device) for d in self.n_latent_encoder] if want_latents else []
        harr, nh = _lib.fptr_array(hs)
        if n > 0:
            self._call(self._lib.iwae_generate(self._h, n, _lib.fptr(h_top), arr, ne, _lib.fptr(ut),
                                               _lib.fptr(probs), ld if want_probs else 0,
                                               _lib.fptr(pixels), ld if want_pixels else 0, harr, nh))
        self._stream.synchronize()
        return (probs[:, :self.x_dim] if want_probs else None, pixels[:, :self.x_dim] if want_pixels else None,
                hs if want_latents else None)

    def generate_x(self, h_top, eps=None):
        """Decoder.generate_x (F:107-F:119): pixel probabilities of the images
        generated from the top latent ``h_top`` ([S, B, d_L] as in the
        reference, or [B, d_L]) by ancestral sampling through the decoder's
        prior layers; device tensor [S, B, x_dim] (or [B, x_dim]).  The rows
        are the flattened S*B.  ``eps``: the L-1 prior draws in generation
        order, [1, S*B, d_{L-2-j}]."""
        with torch.cuda.stream(self._stream):
            t = torch.as_tensor(h_top).to(device=self.device, dtype=torch.float32).contiguous()
        dL = self.n_latent_encoder[-1]
        if t.dim() not in (2, 3) or t.shape[-1] != dL:
            raise ValueError(f"h_top must be [S, B, {dL}] or [B, {dL}], got {tuple(t.shape)}")
        lead = tuple(t.shape[:-1])
        probs, _, _ = self._generate(int(np.prod(lead)), t.reshape(-1, dL), eps, None, True, False, False)
        return probs.reshape(*lead, self.x_dim)

    def sample(self, n, eps=None, u=None, return_probs=True, return_latents=False):
        """n unconditional samples: h_L ~ N(0, I), ancestral sampling down the
        decoder's prior layers (F:107-F:119), binary pixels x ~ Bernoulli(probs).
        Returns {"x": [n, x_dim] of 0.0 / 1.0} plus "probs" ([n, x_dim]) and
        "h" (the L latents [n, d_i], encoder order) when asked for.  ``eps``:
        L arrays [1, n, d], h_L's first and then the prior draws in generation
        order; ``u``: [n, x_dim] uniforms for the pixel draws.  By default all
        noise is drawn on the device (Philox)."""
        probs, pixels, hs = self._generate(n, None, eps, u, bool(return_probs), True, bool(return_latents))
        out = {"x": pixels}
        if return_probs:
            out["probs"] = probs
        if return_latents:
            out["h"] = hs
        return out

    def encoder_means(self, x, n_samples, eps=None):
        """Device [N, d_i] per layer: the mean over n_samples draws of q(h|x)
        of h_i (the accumulation of F:268-F:276).  ``eps``: [n, N, d_i]."""
        xd = self._x(x)
        N = xd.shape[0]
        arr, n, keep = self._eps(eps, N, n_samples)
        with torch.cuda.stream(self._stream):
            outs = [torch.empty(N, d, device=self.device) for d in self.n_latent_encoder]
        oarr, no = _lib.fptr_array(outs)
        self._call(self._lib.iwae_encoder_means(self._h, _lib.fptr(xd), N, int(n_samples), arr, n, oarr, no))
        self._stream.synchronize()
        return outs

    # ------------------------------------------ importance-weighted posterior
    POSTERIOR_OUTPUTS = ("h_mean", "probs", "h_sir", "weights", "ess", "log_px")

    def posterior(self, x, k, eps=None, u=None, chunk=0, want=POSTERIOR_OUTPUTS):
        """The importance-weighted posterior q_IW of each image (iwae_posterior):
        k samples of q(h|x) reweighted by w~ = softmax_k(log w).  Returns a dict of
        device tensors with the entries named in ``want``:

        - ``"weights"`` [N, k]: w~;  ``"log_px"`` [N]: the k-sample log p(x) of
          ``log_px``;  ``"ess"`` [N]: the effective sample size 1 / sum_s w~_s^2;
        - ``"h_mean"``: per stochastic layer [N, d_i], sum_s w~_s h_{i,s};
        - ``"probs"`` [N, x_dim]: sum_s w~_s p(x | h_{1,s}) with h_1 the encoder's
          sample (the quantity log w is made of);
        - ``"h_sir"``: per layer [N, d_i], the latents of one sample per image
          drawn from q_IW by sampling-importance-resampling: sample
          min{j : sum_{s<=j} w~_s > u}.

        ``eps``: L arrays [k, N, d_i] (default: device noise, the stream of
        ``log_px``); ``u``: [N] uniforms in [0, 1) for the resampling (default:
        device noise); ``chunk``: images per chunk (0: automatic)."""
        xd = self._x(x)
        N, k = xd.shape[0], int(k)
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in self.POSTERIOR_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want must name some of {self.POSTERIOR_OUTPUTS}, got {want}")
        if N <= 0 or k <= 0:
            raise ValueError("N and k must be positive")
        if k > 1 << 20:
            raise ValueError("k above 2^20 per image is not supported")
        arr, n, keep = self._eps(eps, N, k)
        ut = None
        if u is not None:
            with torch.cuda.stream(self._stream):
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).contiguous()
            if tuple(ut.shape) != (N,):
                raise ValueError(f"u must be [N={N}], got {tuple(ut.shape)}")
        dims = self.n_latent_encoder
        with torch.cuda.stream(self._stream):
            ld = (self.x_dim + 3) // 4 * 4
            hm = [torch.empty(N, d, device=self.device) for d in dims] if "h_mean" in want else []
            hs = [torch.empty(N, d, device=self.device) for d in dims] if "h_sir" in want else []
            probs = torch.empty(N, ld, device=self.device) if "probs" in want else None
            wts = torch.empty(N, k, device=self.device) if "weights" in want else None
            ess = torch.empty(N, device=self.device) if "ess" in want else None
            lpx = torch.empty(N, device=self.device) if "log_px" in want else None
        marr, nm = _lib.fptr_array(hm)
        sarr, ns = _lib.fptr_array(hs)
        self._call(self._lib.iwae_posterior(self._h, _lib.fptr(xd), N, k, int(chunk), arr, n, _lib.fptr(ut), marr, nm,
                                            _lib.fptr(probs), ld if probs is not None else 0, sarr, ns,
                                            _lib.fptr(wts), _lib.fptr(ess), _lib.fptr(lpx)))
        self._stream.synchronize()
        out = {"h_mean": hm, "h_sir": hs, "probs": probs[:, :self.x_dim] if probs is not None else None,
               "weights": wts, "ess": ess, "log_px": lpx}
        return {name: out[name] for name in want}

    # ------------------------------------------------ scoring given latents
    SCORE_OUTPUTS = ("log_q", "log_ph", "log_px", "probs")

    def _latents(self, h):
        """L latent arrays [n, B, d_i] as contiguous device tensors; (tensors, n, B)."""
        h = list(h)
        dims = self.n_latent_encoder
        if len(h) != len(dims):
            raise ValueError(f"expected {len(dims)} latent arrays (one per stochastic layer), got {len(h)}")
        ts = []
        with torch.cuda.stream(self._stream):
            for i, v in enumerate(h):
                t = torch.as_tensor(v).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
                if t.dim() != 3 or t.shape[2] != dims[i] or (ts and tuple(t.shape[:2]) != tuple(ts[0].shape[:2])):
                    raise ValueError(f"h[{i}] must be [n_samples, B, d={dims[i]}] like the others, got {tuple(t.shape)}")
                ts.append(t)
        return ts, int(ts[0].shape[0]), int(ts[0].shape[1])

    def score(self, x, h, want=("log_q", "log_ph", "log_px"), chunk=0):
        """Densities of caller-supplied latents (iwae_score).  ``h``: L arrays or
        tensors [n_samples, B, d_i] (the reference's layout of h_i).  Returns a
        dict of device tensors with the entries named in ``want``, each
        [n_samples, B] like the reference's: ``"log_q"`` = log q(h|x) (F:60 /
        F:70), ``"log_ph"`` = log p(h) (F:134-F:142), ``"log_px"`` = log p(x|h_1)
        (F:123-F:129); ``"log_w"`` = log_ph + log_px - log_q is added when all
        three are asked for; ``"probs"`` [n_samples, B, x_dim]: p(h_1), the first
        item of the decoder's call.  ``x`` may be None when neither log_q nor
        log_px is asked for.  Nothing is drawn; ``chunk``: images per chunk (0:
        automatic)."""
        return self._score(x, None, h, want, chunk)

    def _score(self, x, mask, h, want, chunk):
        """``score`` (mask None) and ``score_observed``."""
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in self.SCORE_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want must name some of {self.SCORE_OUTPUTS}, got {want}")
        ts, k, B = self._latents(h)
        if B <= 0 or k <= 0:
            raise ValueError("n_samples and B must be positive")
        xd = None
        if x is not None:
            xd = self._x(x)
            if xd.shape[0] != B:
                raise ValueError(f"x has {xd.shape[0]} images, the latents {B}")
        elif "log_q" in want or "log_px" in want:
            raise ValueError("log_q and log_px need x")
        mt = self._observed_mask(mask, xd, B)
        with torch.cuda.stream(self._stream):
            ld = (self.x_dim + 3) // 4 * 4
            terms = {n: torch.empty(B, k, device=self.device) for n in ("log_q", "log_ph", "log_px") if n in want}
            probs = torch.empty(B * k, ld, device=self.device) if "probs" in want else None
        arr, n = _lib.fptr_array(ts)
        outs = (_lib.fptr(terms.get("log_q")), _lib.fptr(terms.get("log_ph")), _lib.fptr(terms.get("log_px")),
                _lib.fptr(probs), ld if probs is not None else 0)
        if mt is None:
            self._call(self._lib.iwae_score(self._h, _lib.fptr(xd), B, k, int(chunk), arr, n, *outs))
        else:
            self._call(self._lib.iwae_score_masked(self._h, _lib.fptr(xd), _lib.fptr(mt), B, k, int(chunk), arr, n, *outs))
        with torch.cuda.stream(self._stream):
            out = {n: t.t().contiguous() for n, t in terms.items()}
            if len(terms) == 3:
                out["log_w"] = (out["log_ph"] + out["log_px"]) - out["log_q"]
            if probs is not None:
                out["probs"] = probs[:, :self.x_dim].reshape(B, k, self.x_dim).transpose(0, 1).contiguous()
        self._stream.synchronize()
        return out

    SCORE_GRAD_OUTPUTS = ("grad", "log_q", "log_ph", "log_px")

    def score_grad(self, x, h, coef=(0.0, 1.0, 1.0), want=("grad",), chunk=0):
        """Gradients of the scored densities with respect to the latents
        (iwae_score_grad).  ``h`` as in ``score``; ``coef`` = (c_q, c_ph, c_px).
        Returns a dict with the entries named in ``want``: ``"grad"``: a list of L
        device tensors shaped like ``h``, grad[i] = c_q dlog q(h|x)/dh_i + c_ph
        dlog p(h)/dh_i + c_px dlog p(x|h_1)/dh_i per row ((0, 1, 1): the posterior
        score; (-1, 1, 1): dlog w/dh); ``"log_q"``, ``"log_ph"``, ``"log_px"``
        [n_samples, B] as ``score`` returns them (``"log_w"`` added when all three
        are asked for).  A term with coefficient 0 is not computed unless its value
        is asked for; ``x`` may be None when neither c_q nor c_px nor their values
        need it.  Nothing is drawn."""
        return self._score_grad(x, None, h, coef, want, chunk)

    def _score_grad(self, x, mask, h, coef, want, chunk):
        """``score_grad`` (mask None) and ``score_grad_observed``."""
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in self.SCORE_GRAD_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want must name some of {self.SCORE_GRAD_OUTPUTS}, got {want}")
        cf = [float(c) for c in coef]
        if len(cf) != 3:
            raise ValueError("coef must be (c_q, c_ph, c_px)")
        ts, k, B = self._latents(h)
        if B <= 0 or k <= 0:
            raise ValueError("n_samples and B must be positive")
        with_g = "grad" in want
        xd = None
        if x is not None:
            xd = self._x(x)
            if xd.shape[0] != B:
                raise ValueError(f"x has {xd.shape[0]} images, the latents {B}")
        elif "log_q" in want or "log_px" in want or (with_g and (cf[0] != 0.0 or cf[2] != 0.0)):
            raise ValueError("log q and log p(x|h), values or gradient terms, need x")
        mt = self._observed_mask(mask, xd, B)
        with torch.cuda.stream(self._stream):
            terms = {n: torch.empty(B, k, device=self.device) for n in ("log_q", "log_ph", "log_px") if n in want}
            gs = [torch.empty_like(t) for t in ts] if with_g else []
        arr, n = _lib.fptr_array(ts)
        garr, ng = _lib.fptr_array(gs)
        carr = (ctypes.c_float * 3)(*cf)
        outs = (_lib.fptr(terms.get("log_q")), _lib.fptr(terms.get("log_ph")), _lib.fptr(terms.get("log_px")))
        if mt is None:
            self._call(self._lib.iwae_score_grad(self._h, _lib.fptr(xd), B, k, int(chunk), arr, n, carr, garr, ng, *outs))
        else:
            self._call(self._lib.iwae_score_grad_masked(self._h, _lib.fptr(xd), _lib.fptr(mt), B, k, int(chunk), arr, n,
                                                        carr, garr, ng, *outs))
        with torch.cuda.stream(self._stream):
            out = {n: t.t().contiguous() for n, t in terms.items()}
            if len(terms) == 3:
                out["log_w"] = (out["log_ph"] + out["log_px"]) - out["log_q"]
            if with_g:
                out["grad"] = gs
        self._stream.synchronize()
        return out

    def hmc(self, x, h, step_size, n_leapfrog, n_iter=1, momentum=None, u=None, chunk=0):
        """Metropolis-adjusted HMC on the latents with target p(h|x) ~ p(x, h)
        (Hoffman 2017).  Every row (sample s, image b) of ``h`` is a chain of its
        own, all layers move jointly, the mass matrix is the identity.  One
        iteration: momenta r ~ N(0, I); ``n_leapfrog`` leapfrog steps (half kick
        r += eps/2 g, drift h += eps r, half kick) with g = ``score_grad(coef=(0,
        1, 1))``; accept iff log u < H_old - H_new, H = -(log_ph + log_px) + |r|^2
        / 2.  ``momentum``: per iteration a list of L arrays [n_samples, B, d_i];
        ``u``: [n_iter, n_samples, B] uniforms in (0, 1); when absent they are
        drawn from a ``torch.Generator`` on the device seeded with the model's seed
        (the constructor's, or the last ``set_seed``'s) that persists across calls,
        momenta first, then u, per iteration.  The gradient and the densities run
        in the library; the elementwise steps are torch ops on device tensors.
        Returns (h_new: list of L device tensors, accept: bool [n_samples, B] of
        the last iteration, mean acceptance rate over chains and iterations,
        log p(x, h_new) [n_samples, B]); ``self.hmc_info`` keeps the last
        iteration's proposal and its H_old / H_new per chain (diagnostics)."""
        return self._hmc(x, None, h, step_size, n_leapfrog, n_iter, momentum, u, chunk)

    def _hmc(self, x, mask, h, step_size, n_leapfrog, n_iter, momentum, u, chunk):
        """``hmc`` (mask None) and ``hmc_observed``."""
        n_leapfrog, n_iter = int(n_leapfrog), int(n_iter)
        if n_leapfrog <= 0 or n_iter <= 0:
            raise ValueError("n_leapfrog and n_iter must be positive")
        eps = float(step_size)
        ts, k, B = self._latents(h)
        xd = self._x(x)
        mt = self._observed_mask(mask, xd, xd.shape[0])
        if momentum is not None and len(momentum) != n_iter:
            raise ValueError(f"momentum must hold {n_iter} lists (one per iteration)")
        if self._hmc_gen is None and (momentum is None or u is None):
            self._hmc_gen = torch.Generator(device=self.device)
            self._hmc_gen.manual_seed(self._seed & ((1 << 63) - 1))
        VALS = ("grad", "log_ph", "log_px")

        def joint(hs):
            o = self._score_grad(xd, mt, hs, (0.0, 1.0, 1.0), VALS, chunk)
            return o["grad"], o["log_ph"] + o["log_px"]

        with torch.cuda.stream(self._stream):
            cur = [t.clone() for t in ts]
            if u is not None:
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).reshape(n_iter, k, B)
        g_cur, lp_cur = joint(cur)
        acc_sum = 0.0
        acc = None
        for it in range(n_iter):
            with torch.cuda.stream(self._stream):
                if momentum is not None:
                    r = [t.clone() for t in self._latents(momentum[it])[0]]
                    if tuple(r[0].shape[:2]) != (k, B):
                        raise ValueError("momentum must be shaped like h")
                else:
                    r = [torch.randn(t.shape, device=self.device, generator=self._hmc_gen) for t in cur]
                lu = torch.log(ut[it] if u is not None
                               else torch.rand(k, B, device=self.device, generator=self._hmc_gen))
                h_old = -lp_cur + 0.5 * sum((v * v).sum(-1) for v in r)
                q = [t.clone() for t in cur]
                g = g_cur
            for step in range(n_leapfrog):
                with torch.cuda.stream(self._stream):
                    for i in range(len(q)):
                        r[i] += (0.5 * eps) * g[i]
                        q[i] += eps * r[i]
                g, lp = joint(q)
                with torch.cuda.stream(self._stream):
                    for i in range(len(q)):
                        r[i] += (0.5 * eps) * g[i]
            with torch.cuda.stream(self._stream):
                h_new = -lp + 0.5 * sum((v * v).sum(-1) for v in r)
                acc = lu < (h_old - h_new)                        # a NaN proposal is rejected
                sel = acc.unsqueeze(-1)
                cur = [torch.where(sel, a, b) for a, b in zip(q, cur)]
                g_cur = [torch.where(sel, a, b) for a, b in zip(g, g_cur)]
                lp_cur = torch.where(acc, lp, lp_cur)
                acc_sum += float(acc.float().mean())
            self.hmc_info = {"proposal": q, "h_old": h_old, "h_new": h_new}
        self._stream.synchronize()
        return cur, acc, acc_sum / n_iter, lp_cur

    def ais(self, x, k, betas=None, n_temps=1000, init="prior", h0=None, step_size=0.1, n_leapfrog=10,
            adapt=(1.02, 0.98, 1e-4, 1.0), momentum=None, u=None, step=None, chunk=0):
        """Annealed importance sampling of log p(x) (iwae_ais; Wu et al. 2017): k
        chains per image, each a row (sample s, image b), run through the
        schedule ``betas`` (default ``ais_schedule(n_temps)``; any values in
        [0, 1]: ascending from 0 to 1 is AIS, descending from 1 the reverse chain
        of bidirectional Monte Carlo, constant 1 plain HMC on p(h|x)) by
        Metropolis-adjusted HMC transitions of ``n_leapfrog`` leapfrog steps,
        entirely on the device.  ``init="prior"`` anneals from p(h) to p(x, h),
        ``init="q"`` from q(h|x).  Initial latents: ``h0`` (L arrays [k, B, d_i],
        as ``score`` takes; e.g. ``sample(return_latents=True)["h"]`` reshaped,
        for a reverse chain), else the encoder's samples (``init="q"``) or
        ancestral samples of the prior (``init="prior"``), both on device noise.
        Every chain has its own step size, ``step_size`` at first (or ``step``
        [k, B]), multiplied by ``adapt[0]`` after an accepted and ``adapt[1]``
        after a rejected transition and kept in [``adapt[2]``, ``adapt[3]``].
        ``momentum``: per transition a list of L arrays [k, B, d_i]; ``u``:
        [T, k, B] uniforms in (0, 1); absent, both are device noise (Philox,
        the stream ``set_seed`` positions).  Returns a dict of device tensors:
        ``"logpx"`` [B] = logsumexp_s log_w - log k, ``"log_w"`` [k, B],
        ``"ess"`` [B], ``"h"`` (the L final latents [k, B, d_i]),
        ``"accept_rate"`` [k, B] and ``"step"`` [k, B] (the final step sizes).
        The chain itself never waits for the host; the call synchronizes once,
        at the end (drawing the initial latents is a call of its own)."""
        return self._ais(x, None, k, betas, n_temps, init, h0, step_size, n_leapfrog, adapt, momentum, u, step, chunk)

    def _ais(self, x, mask, k, betas, n_temps, init, h0, step_size, n_leapfrog, adapt, momentum, u, step, chunk):
        """``ais`` (mask None) and ``ais_observed``."""
        if init not in ("prior", "q"):
            raise ValueError('init must be "prior" or "q"')
        xd = self._x(x)
        B, k = xd.shape[0], int(k)
        if B <= 0 or k <= 0:
            raise ValueError("B and k must be positive")
        mt = self._observed_mask(mask, xd, B)
        bt = np.ascontiguousarray(ais_schedule(int(n_temps)) if betas is None else betas, dtype=np.float32).ravel()
        T = bt.size - 1
        n_leapfrog = int(n_leapfrog)
        if T < 1 or n_leapfrog < 1:
            raise ValueError("betas must hold at least two values and n_leapfrog must be positive")
        if len(adapt) != 4:
            raise ValueError("adapt must be (inc, dec, step_min, step_max)")
        dims = self.n_latent_encoder
        L = len(dims)
        if h0 is not None:
            ts, kk, BB = self._latents(h0)
            if (kk, BB) != (k, B):
                raise ValueError(f"h0 must be [k={k}, B={B}, d_i] per layer, got [{kk}, {BB}, d_i]")
            with torch.cuda.stream(self._stream):
                hs = [t.clone() for t in ts]
        elif init == "q":
            hs = self._encode(self._observed_x(xd, mt), k, chunk=chunk)[0]
        else:
            # (iwae_generate wants an image output: the probabilities, which draw nothing more)
            hs = [t.reshape(k, B, d) for t, d in zip(self._generate(k * B, None, None, None, True, False, True)[2], dims)]
        keep = []
        marr, nm = None, 0
        if momentum is not None:
            if len(momentum) != T:
                raise ValueError(f"momentum must hold {T} lists (one per transition)")
            for r in momentum:
                rs, kk, BB = self._latents(r)
                if (kk, BB) != (k, B):
                    raise ValueError("momentum must be shaped like the latents")
                keep += rs
            marr, nm = _lib.fptr_array(keep)
        ut = st = None
        with torch.cuda.stream(self._stream):
            if u is not None:
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32)
                if tuple(ut.shape) != (T, k, B):
                    raise ValueError(f"u must be [T={T}, k={k}, B={B}], got {tuple(ut.shape)}")
                ut = ut.transpose(1, 2).contiguous()
            if step is not None:
                st = torch.as_tensor(step).to(device=self.device, dtype=torch.float32)
                if tuple(st.shape) != (k, B):
                    raise ValueError(f"step must be [k={k}, B={B}], got {tuple(st.shape)}")
                st = st.t().contiguous()
            else:
                st = torch.full((B, k), float(step_size), device=self.device)
            lw = torch.empty(B, k, device=self.device)
            acc = torch.empty(B, k, device=self.device)
            lpx = torch.empty(B, device=self.device)
            ess = torch.empty(B, device=self.device)
        cfg = _lib.IwaeAisConfig(init=0 if init == "prior" else 1, n_temps=T, n_leapfrog=n_leapfrog, accumulate=0,
                                 step=float(step_size), adapt_inc=float(adapt[0]), adapt_dec=float(adapt[1]),
                                 step_min=float(adapt[2]), step_max=float(adapt[3]))
        harr, nh = _lib.fptr_array(hs)
        tail = (harr, nh, ctypes.byref(cfg), bt.ctypes.data_as(_lib.FP), marr, nm, _lib.fptr(ut), _lib.fptr(st),
                _lib.fptr(lw), _lib.fptr(acc), _lib.fptr(lpx), _lib.fptr(ess))
        if mt is None:
            self._call(self._lib.iwae_ais(self._h, _lib.fptr(xd), B, k, int(chunk), *tail))
        else:
            self._call(self._lib.iwae_ais_masked(self._h, _lib.fptr(xd), _lib.fptr(mt), B, k, int(chunk), *tail))
        with torch.cuda.stream(self._stream):
            out = {"logpx": lpx, "log_w": lw.t().contiguous(), "ess": ess, "h": hs,
                   "accept_rate": (acc / T).t().contiguous(), "step": st.t().contiguous()}
        self._stream.synchronize()
        return out

    REFINE_OUTPUTS = ("bound", "log_w", "logpx", "ess", "h")

    def _encoder_gaussian(self, xd):
        """(means, logstds), L device tensors [B, d_i] each: the encoder's mean chain
        (h_i at zero noise) and its scales along it, from iwae_encode alone."""
        B = xd.shape[0]
        dims = self.n_latent_encoder
        L = len(dims)
        if L == 1:
            _, _, top = self._encode(xd, 1, eps=[np.zeros((1, B, dims[0]), np.float32)])
            with torch.cuda.stream(self._stream):
                return [top.loc.clone()], [torch.log(top.scale)]
        # sample 0: no noise; sample j: unit noise at layer j only, so h_j moves by exactly its scale
        eps = [np.zeros((L + 1, B, d), np.float32) for d in dims]
        for j in range(L):
            eps[j][j + 1] = 1.0
        hs, _, _ = self._encode(xd, L + 1, eps=eps)
        with torch.cuda.stream(self._stream):
            return [h[0].clone() for h in hs], [torch.log(h[j + 1] - h[0]) for j, h in enumerate(hs)]

    def refine(self, x, k, n_iters=100, objective="ELBO", lr=0.01, betas=(0.9, 0.999), epsilon=1e-7,
               logstd_range=(-12.0, 4.0), init="encoder", state=None, eps=None, chunk=0, want=REFINE_OUTPUTS):
        """Per-image variational refinement (iwae_refine; Cremer, Li & Duvenaud
        2018): ``n_iters`` Adam ascent steps on one diagonal Gaussian per image
        over all latent layers, q*(h) = prod_i N(h_i; m_i, exp(ls_i)^2), with k
        reparameterised samples per image and step, entirely on the device.
        ``objective``: ``"ELBO"`` (mean_s log w_s) or ``"IWAE"`` (logsumexp_s log
        w_s - log k).  ``init``: ``"encoder"`` (the encoder's mean chain and its
        scales along it, one ``encoder`` call) or a pair ``(means, logstds)`` of L
        arrays [B, d_i] each (copied).  ``lr``, ``betas``, ``epsilon``: Adam's;
        the log standard deviations are kept in ``logstd_range``.  After the
        updates one evaluation pass draws k fresh samples at the final parameters
        when ``want`` names any of ``"log_w"`` [k, B], ``"logpx"`` [B] =
        logsumexp_s log_w - log k (at ELBO-optimal q* and large k: the estimate
        whose distance to ``ais`` is the approximation gap), ``"ess"`` [B] and
        ``"h"`` (the L sample tensors [k, B, d_i]); ``"bound"`` [n_iters, B] is
        the objective before each update on that step's samples.  ``n_iters=0``
        only evaluates the given q*.  ``eps``: per pass (the ``n_iters`` steps,
        then the evaluation if there is one) a list of L arrays [k, B, d_i];
        absent: device noise (Philox, the stream ``set_seed`` positions).
        Returns a dict of device tensors: ``"mean"``, ``"logstd"`` (lists of [B,
        d_i]), the entries of ``want``, and ``"state"`` (Adam's moments and step
        count), which ``state=`` takes back, together with ``init=(out["mean"],
        out["logstd"])``, to continue the run: two such calls give bit for bit
        what one call over all the steps gives when the first evaluated nothing
        (``want=("bound",)``).  The call synchronizes once, at the end."""
        return self._refine(x, None, k, n_iters, objective, lr, betas, epsilon, logstd_range, init, state, eps, chunk, want)

    def _refine(self, x, mask, k, n_iters, objective, lr, betas, epsilon, logstd_range, init, state, eps, chunk, want):
        """``refine`` (mask None) and ``refine_observed``."""
        if objective not in ("ELBO", "IWAE"):
            raise ValueError('objective must be "ELBO" or "IWAE"')
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in self.REFINE_OUTPUTS]
        if bad:
            raise ValueError(f"want must name some of {self.REFINE_OUTPUTS}, got {want}")
        xd = self._x(x)
        B, k, T = xd.shape[0], int(k), int(n_iters)
        if B <= 0 or k <= 0 or T < 0:
            raise ValueError("B and k must be positive, n_iters non-negative")
        mt = self._observed_mask(mask, xd, B)
        if len(betas) != 2 or len(logstd_range) != 2:
            raise ValueError("betas must be (beta1, beta2), logstd_range (min, max)")
        dims = self.n_latent_encoder
        L = len(dims)
        if isinstance(init, str):
            if init != "encoder":
                raise ValueError('init must be "encoder" or a (means, logstds) pair')
            mean, logstd = self._encoder_gaussian(self._observed_x(xd, mt))
        else:
            if len(init) != 2 or len(init[0]) != L or len(init[1]) != L:
                raise ValueError(f"init must be (means, logstds), {L} arrays [B, d_i] each")
            with torch.cuda.stream(self._stream):
                mean, logstd = ([torch.as_tensor(v).to(device=self.device, dtype=torch.float32).clone().contiguous()
                                 for v in part] for part in init)
            for t, d in zip(mean + logstd, list(dims) * 2):
                if tuple(t.shape) != (B, d):
                    raise ValueError(f"init arrays must be [B={B}, d_i], got {tuple(t.shape)} for d_i = {d}")
        evaluate = any(w in want for w in ("log_w", "logpx", "ess", "h"))
        if T == 0 and not evaluate:
            raise ValueError("n_iters = 0 with no evaluation output has nothing to do")
        P = T + (1 if evaluate else 0)
        keep = []
        if eps is not None:
            if len(eps) != P:
                raise ValueError(f"eps must hold {P} lists (one per step, then the evaluation's)")
            for e in eps:
                es, kk, BB = self._latents(e)
                if (kk, BB) != (k, B):
                    raise ValueError(f"eps arrays must be [k={k}, B={B}, d_i]")
                keep += es
        earr, ne = _lib.fptr_array(keep)
        step0 = 0
        with torch.cuda.stream(self._stream):
            if state is not None:
                step0, adam = int(state["step"]), list(state["adam"])
                if len(adam) != 4 * L or any(tuple(t.shape) != (B, dims[i // 4]) for i, t in enumerate(adam)):
                    raise ValueError("state does not belong to a run on these images")
            else:
                adam = [torch.empty(B, d, device=self.device) for d in dims for _ in range(4)]
            bound = torch.empty(T, B, device=self.device) if "bound" in want and T > 0 else None
            hs = [torch.empty(k, B, d, device=self.device) for d in dims] if "h" in want else []
            lw = torch.empty(B, k, device=self.device) if "log_w" in want else None
            lpx = torch.empty(B, device=self.device) if "logpx" in want else None
            ess = torch.empty(B, device=self.device) if "ess" in want else None
        cfg = _lib.IwaeRefineConfig(objective=0 if objective == "ELBO" else 1, n_iters=T, step0=step0, lr=float(lr),
                                    beta1=float(betas[0]), beta2=float(betas[1]), epsilon=float(epsilon),
                                    logstd_min=float(logstd_range[0]), logstd_max=float(logstd_range[1]))
        marr, nm = _lib.fptr_array(mean)
        sarr, _ = _lib.fptr_array(logstd)
        aarr, na = _lib.fptr_array(adam)
        harr, nh = _lib.fptr_array(hs)
        tail = (marr, sarr, nm, ctypes.byref(cfg), earr, ne, aarr, na, _lib.fptr(bound), harr, nh, _lib.fptr(lw),
                _lib.fptr(lpx), _lib.fptr(ess))
        if mt is None:
            self._call(self._lib.iwae_refine(self._h, _lib.fptr(xd), B, k, int(chunk), *tail))
        else:
            self._call(self._lib.iwae_refine_masked(self._h, _lib.fptr(xd), _lib.fptr(mt), B, k, int(chunk), *tail))
        out = {"mean": mean, "logstd": logstd, "state": {"adam": adam, "step": step0 + T}}
        with torch.cuda.stream(self._stream):
            if "bound" in want:
                out["bound"] = bound if bound is not None else torch.empty(0, B, device=self.device)
            if lw is not None:
                out["log_w"] = lw.t().contiguous()
            if lpx is not None:
                out["logpx"] = lpx
            if ess is not None:
                out["ess"] = ess
            if hs:
                out["h"] = hs
        self._stream.synchronize()
        return out

    def _encode(self, x, n_samples, eps=None, chunk=0):
        """iwae_encode behind ``model.encoder(x, n_samples)``."""
        xd = self._x(x)
        B, k = xd.shape[0], int(n_samples)
        if B <= 0 or k <= 0:
            raise ValueError("B and n_samples must be positive")
        arr, n, keep = self._eps(eps, B, k)
        dims = self.n_latent_encoder
        L = len(dims)
        with torch.cuda.stream(self._stream):
            hs = [torch.empty(k, B, d, device=self.device) for d in dims]
            lq = torch.empty(B, k, device=self.device)
            top = (B, dims[0]) if L == 1 else (k, B, dims[-1])
            loc = torch.empty(*top, device=self.device)
            scale = torch.empty(*top, device=self.device)
        harr, nh = _lib.fptr_array(hs)
        self._call(self._lib.iwae_encode(self._h, _lib.fptr(xd), B, k, int(chunk), arr, n, harr, nh, _lib.fptr(lq),
                                         _lib.fptr(loc), _lib.fptr(scale)))
        with torch.cuda.stream(self._stream):
            lq = lq.t().contiguous()
        self._stream.synchronize()
        return hs, lq, _Normal(loc, scale)

    # ------------------------------------------------- aggregate posterior
    def log_q_aggregate(self, h1, x_ref=None, loc=None, scale=None, own_period=0, want=("log_q_agg",), chunk=0):
        """The aggregate posterior q(h_1) = 1/M sum_m q(h_1 | x_m) at the latents
        ``h1`` ([R, d1] or [k, N, d1]; iwae_aggregate).  The M components are the
        first encoder layer's Gaussians of ``x_ref`` [M, x_dim], or the caller's
        ``loc`` / ``scale`` [M, d1] (exactly one of the two forms).  Returns a
        dict of device tensors with the entries named in ``want``, shaped like
        ``h1`` without (log_q_agg, log_q_own) or with (log_q_dim, log_q_own_dim)
        its last axis; ``"loc"`` / ``"scale"`` [M, d1]: the components used.
        ``own_period`` P > 0: row r's own image is r mod P (for [k, N, d1]
        latents of x_ref itself: P = N).  Nothing is drawn."""
        d1 = self.n_latent_encoder[0]
        with torch.cuda.stream(self._stream):
            ht = torch.as_tensor(h1).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
            lt = st = None
            if loc is not None:
                lt = torch.as_tensor(loc).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
            if scale is not None:
                st = torch.as_tensor(scale).to(device=self.device, dtype=torch.float32, non_blocking=True).contiguous()
        xd = self._x(x_ref) if x_ref is not None else None
        comp = [tuple(t.shape) for t in (lt, st) if t is not None]
        M = int(xd.shape[0]) if xd is not None else (comp[0][0] if comp and len(comp[0]) == 2 else 0)
        R, want = check_aggregate_args(tuple(ht.shape), d1, xd is not None, comp, M, own_period, want)
        lead = tuple(ht.shape[:-1])
        with torch.cuda.stream(self._stream):
            if xd is not None:
                lt = torch.empty(M, d1, device=self.device) if "loc" in want else None
                st = torch.empty(M, d1, device=self.device) if "scale" in want else None
            out = {n: torch.empty(*lead, device=self.device) for n in ("log_q_agg", "log_q_own") if n in want}
            out.update({n: torch.empty(*lead, d1, device=self.device) for n in ("log_q_dim", "log_q_own_dim") if n in want})
        self._call(self._lib.iwae_aggregate(
            self._h, _lib.fptr(xd), M, int(chunk), _lib.fptr(lt), _lib.fptr(st), _lib.fptr(ht), R, int(own_period),
            _lib.fptr(out.get("log_q_agg")), _lib.fptr(out.get("log_q_dim")), _lib.fptr(out.get("log_q_own")),
            _lib.fptr(out.get("log_q_own_dim"))))
        if "loc" in want:
            out["loc"] = lt
        if "scale" in want:
            out["scale"] = st
        self._stream.synchronize()
        return out

    def aggregate_posterior(self, x, k, x_ref=None, eps=None, chunk=0, per_unit=False):
        """k samples per image of q(h|x) (``model.encoder``'s draw: the samples a
        layer-wise ``get_log_weights`` of the same seed weighs) scored under the
        aggregate posterior of ``x_ref`` (default: x itself, and then also under
        each row's own image).  Returns a dict of device tensors, image-major
        [N, k]: ``log_q`` = log q(h|x), ``log_ph`` = log p(h), ``log_q_agg`` =
        log q(h_1), with x_ref None ``log_q_own`` = log q(h_1|x); ``per_unit``
        adds ``log_q_dim`` (and ``log_q_own_dim``) [N, k, d1]; ``h``: the latents,
        L tensors [k, N, d_i]."""
        hs, lq, _ = self._encode(x, k, eps=eps, chunk=chunk)
        N = int(hs[0].shape[1])
        lp = self._score(None, None, hs, ("log_ph",), chunk)["log_ph"]
        own = x_ref is None
        want = ["log_q_agg"] + (["log_q_own"] if own else [])
        if per_unit:
            want += ["log_q_dim"] + (["log_q_own_dim"] if own else [])
        agg = self.log_q_aggregate(hs[0], x_ref=x if own else x_ref, own_period=N if own else 0, want=want, chunk=chunk)
        with torch.cuda.stream(self._stream):
            out = {"log_q": lq.t().contiguous(), "log_ph": lp.t().contiguous()}
            out.update({n: t.transpose(0, 1).contiguous() for n, t in agg.items()})
        out["h"] = hs
        self._stream.synchronize()
        return out

    def information_statistics(self, x, k, eps=None, chunk=0, per_unit=True):
        """ELBO surgery (Hoffman & Johnson 2016) over the data set x with k
        samples per image; means over all N k rows, accumulated in float64 on
        the host:  ``kl`` = mean(log q(h|x) - log p(h));  ``mi`` = mean(log
        q(h_1|x) - log q(h_1)), the full-batch estimate of I_q(x; h), at most
        log N;  ``marginal_kl`` = mean(log q(h|x) - log q(h_1|x) + log q(h_1) -
        log p(h)) = KL(q(h) || p(h)), so mi + marginal_kl == kl;  with
        ``per_unit`` ``total_correlation`` = mean(log q(h_1) - sum_j log
        q_j(h_1j)) and ``mi_per_unit`` [d1] (Chen et al. 2018)."""
        a = self.aggregate_posterior(x, k, eps=eps, chunk=chunk, per_unit=per_unit)
        f = {n: t.double().cpu().numpy() for n, t in a.items() if n != "h"}
        res = dict(kl=float((f["log_q"] - f["log_ph"]).mean()),
                   mi=float((f["log_q_own"] - f["log_q_agg"]).mean()),
                   marginal_kl=float((f["log_q"] - f["log_q_own"] + f["log_q_agg"] - f["log_ph"]).mean()))
        if per_unit:
            res["total_correlation"] = float((f["log_q_agg"] - f["log_q_dim"].sum(-1)).mean())
            res["mi_per_unit"] = (f["log_q_own_dim"] - f["log_q_dim"]).mean((0, 1))
        return res

    def reconstructed_x_probs_iw(self, x, k, eps=None):
        """Importance-weighted reconstruction [N, x_dim]: sum_s w~_s p(x | h_{1,s})
        over k samples of q(h|x) (``posterior(...)["probs"]``)."""
        return self.posterior(x, k, eps=eps, want=("probs",))["probs"]

    # ------------------------------------------- imputation of missing pixels
    IMPUTE_OUTPUTS = ("x_mean", "x_draw", "h_mean", "h_sir", "weights", "ess", "log_px")

    def impute(self, x, mask, k, eps=None, u=None, u_pix=None, chunk=0, want=IMPUTE_OUTPUTS):
        """Missing-pixel imputation under the importance-weighted posterior
        (iwae_impute; Mattei & Frellsen 2019).  ``mask`` [N, x_dim] (or x's
        shape): non-zero = observed, 0 = missing; whatever ``x`` holds at a missing
        pixel is ignored (NaN included).  The encoder sees x * mask, the log
        weights use the likelihood of the observed pixels alone.  Returns a dict
        of device tensors with the entries named in ``want``:

        - ``"x_mean"`` [N, x_dim]: x where observed, sum_s w~_s p(x | h_{1,s})
          where missing (the single imputation E[x_miss | x_obs]);
        - ``"x_draw"`` [N, x_dim]: x where observed, one Bernoulli draw from
          p(x | h_1 of the resampled sample) where missing (one multiple-imputation
          draw; call again with another ``u`` / ``u_pix`` for more);
        - ``"log_px"`` [N]: the k-sample estimate of log p(x_obs); ``"weights"``,
          ``"ess"``, ``"h_mean"``, ``"h_sir"`` as in ``posterior``.

        ``eps``: L arrays [k, N, d_i]; ``u``: [N] uniforms for the resampling;
        ``u_pix``: [N, x_dim] uniforms for the pixel draws (defaults: device
        noise); ``chunk``: images per chunk (0: automatic)."""
        xd = self._x(x)
        N, k = xd.shape[0], int(k)
        want = (want,) if isinstance(want, str) else tuple(want)
        bad = [w for w in want if w not in self.IMPUTE_OUTPUTS]
        if bad or not want:
            raise ValueError(f"want must name some of {self.IMPUTE_OUTPUTS}, got {want}")
        if N <= 0 or k <= 0:
            raise ValueError("N and k must be positive")
        if k > 1 << 20:
            raise ValueError("k above 2^20 per image is not supported")
        if mask is None:
            raise ValueError("mask is required (an all-observed call is posterior's)")
        with torch.cuda.stream(self._stream):
            mt = torch.as_tensor(mask).to(device=self.device, dtype=torch.float32).contiguous()
        if mt.dim() < 2 or mt.shape[0] != N or mt.numel() != N * self.x_dim:
            raise ValueError(f"mask must be [N={N}, {self.x_dim}], got {tuple(mt.shape)}")
        mt = mt.reshape(N, self.x_dim)
        arr, n, keep = self._eps(eps, N, k)
        ut = up = None
        with torch.cuda.stream(self._stream):
            if u is not None:
                ut = torch.as_tensor(u).to(device=self.device, dtype=torch.float32).contiguous()
            if u_pix is not None:
                up = torch.as_tensor(u_pix).to(device=self.device, dtype=torch.float32).contiguous()
        if ut is not None and tuple(ut.shape) != (N,):
            raise ValueError(f"u must be [N={N}], got {tuple(ut.shape)}")
        if up is not None and tuple(up.shape) != (N, self.x_dim):
            raise ValueError(f"u_pix must be [N={N}, {self.x_dim}], got {tuple(up.shape)}")
        dims = self.n_latent_encoder
        with torch.cuda.stream(self._stream):
            ld = (self.x_dim + 3) // 4 * 4
            hm = [torch.empty(N, d, device=self.device) for d in dims] if "h_mean" in want else []
            hs = [torch.empty(N, d, device=self.device) for d in dims] if "h_sir" in want else []
            xm = torch.empty(N, ld, device=self.device) if "x_mean" in want else None
            xw = torch.empty(N, ld, device=self.device) if "x_draw" in want else None
            wts = torch.empty(N, k, device=self.device) if "weights" in want else None
            ess = torch.empty(N, device=self.device) if "ess" in want else None
            lpx = torch.empty(N, device=self.device) if "log_px" in want else None
        marr, nm = _lib.fptr_array(hm)
        sarr, ns = _lib.fptr_array(hs)
        self._call(self._lib.iwae_impute(self._h, _lib.fptr(xd), _lib.fptr(mt), N, k, int(chunk), arr, n,
                                         _lib.fptr(ut), _lib.fptr(up), _lib.fptr(xm), ld if xm is not None else 0,
                                         _lib.fptr(xw), ld if xw is not None else 0, marr, nm, sarr, ns,
                                         _lib.fptr(wts), _lib.fptr(ess), _lib.fptr(lpx)))
        self._stream.synchronize()
        out = {"x_mean": xm[:, :self.x_dim] if xm is not None else None,
               "x_draw": xw[:, :self.x_dim] if xw is not None else None,
               "h_mean": hm, "h_sir": hs, "weights": wts, "ess": ess, "log_px": lpx}
        return {name: out[name] for name in want}

    def log_px_observed(self, x, mask, k=5000, eps=None, chunk=0):
        """The k-sample estimate of log p(x_obs) per image, device [N]
        (``impute(..., want="log_px")["log_px"]``)."""
        return self.impute(x, mask, k, eps=eps, chunk=chunk, want="log_px")["log_px"]

    # ---- inference on caller-controlled latents for incomplete images: the model of ``impute`` and
    # ``train_step(mask=)`` (the encoder sees x where observed and 0 elsewhere, log p(x|h_1) sums the
    # observed pixels, whatever x holds at a missing pixel is ignored, NaN included)
    def _observed_mask(self, mask, xd, B):
        """None for an unmasked call; else the device mask of an ``*_observed`` call."""
        if mask is None:
            return None
        if xd is None:
            raise ValueError("a pixel mask needs x")
        return self._mask(mask, B)

    def _observed_x(self, xd, mt):
        """What the encoder sees: x where observed, 0 where missing (x itself without a mask)."""
        if mt is None:
            return xd
        with torch.cuda.stream(self._stream):
            return torch.where(mt != 0, xd, torch.zeros_like(xd))

    @staticmethod
    def _need_mask(mask):
        if mask is None:
            raise ValueError("mask is required (an all-observed call is the unmasked method's)")

    def score_observed(self, x, mask, h, want=("log_q", "log_ph", "log_px"), chunk=0):
        """``score`` for incomplete images (iwae_score_masked).  ``mask`` [B, x_dim]
        (or x's shape): non-zero = observed.  ``"log_q"`` is log q(h | x where
        observed, 0 elsewhere), ``"log_px"`` sums the observed pixels (exactly 0 for
        an image with none), ``"log_ph"`` is ``score``'s; ``"probs"`` are the
        probabilities of every pixel, observed or not.  Outputs and keys are
        ``score``'s; ``x`` is required."""
        self._need_mask(mask)
        if x is None:
            raise ValueError("x is required")
        return self._score(x, mask, h, want, chunk)

    def score_grad_observed(self, x, mask, h, coef=(0.0, 1.0, 1.0), want=("grad",), chunk=0):
        """``score_grad`` for incomplete images (iwae_score_grad_masked): the
        densities are ``score_observed``'s, a missing pixel pulls on nothing (an
        image with no observed pixel has a zero likelihood gradient).  Outputs
        and keys are ``score_grad``'s; ``x`` is required."""
        self._need_mask(mask)
        if x is None:
            raise ValueError("x is required")
        return self._score_grad(x, mask, h, coef, want, chunk)

    def hmc_observed(self, x, mask, h, step_size, n_leapfrog, n_iter=1, momentum=None, u=None, chunk=0):
        """``hmc`` with target p(h | x_obs): its torch steps on
        ``score_grad_observed``.  Returns what ``hmc`` returns."""
        self._need_mask(mask)
        return self._hmc(x, mask, h, step_size, n_leapfrog, n_iter, momentum, u, chunk)

    def ais_observed(self, x, mask, k, betas=None, n_temps=1000, init="prior", h0=None, step_size=0.1, n_leapfrog=10,
                     adapt=(1.02, 0.98, 1e-4, 1.0), momentum=None, u=None, step=None, chunk=0):
        """``ais`` for incomplete images (iwae_ais_masked): annealed importance
        sampling of log p(x_obs).  With ``init="q"`` and no ``h0`` the initial
        latents are the encoder's samples at x where observed, 0 elsewhere.
        Every other parameter, and the returned dict, are ``ais``'s."""
        self._need_mask(mask)
        return self._ais(x, mask, k, betas, n_temps, init, h0, step_size, n_leapfrog, adapt, momentum, u, step, chunk)

    def refine_observed(self, x, mask, k, n_iters=100, objective="ELBO", lr=0.01, betas=(0.9, 0.999), epsilon=1e-7,
                        logstd_range=(-12.0, 4.0), init="encoder", state=None, eps=None, chunk=0, want=REFINE_OUTPUTS):
        """``refine`` for incomplete images (iwae_refine_masked): q* is fitted to
        p(h | x_obs).  ``init="encoder"`` starts from the encoder's Gaussian at x
        where observed, 0 elsewhere; a continued run passes the same mask.
        Every other parameter, and the returned dict, are ``refine``'s."""
        self._need_mask(mask)
        return self._refine(x, mask, k, n_iters, objective, lr, betas, epsilon, logstd_range, init, state, eps, chunk,
                            want)

    def get_levels_of_units_activity(self, x, n_samples, eps=None):
        """F:264-F:281: per stochastic layer, the variance over the batch of
        E_q[h_i] and the PCA eigenvalues of those means (host float64 on the
        [N, d_i] means the device produced)."""
        means = [m.double().cpu().numpy() for m in self.encoder_means(x, n_samples, eps)]
        variances = [m.var(0) for m in means]
        return variances, [self.get_eigenvalues_PCA(m) for m in means]

    @staticmethod
    def get_eigenvalues_PCA(data):
        """F:284-F:291: ascending eigenvalues of the empirical covariance
        (divisor N) of data [N, D]."""
        d = np.asarray(data, dtype=np.float64)
        z = d - d.mean(0)
        return np.linalg.eigvalsh(z.T @ z / d.shape[0])

    @staticmethod
    def get_active_units(variances, eigen_values, threshold=0.01):
        """F:294-F:300: 0/1 activity per unit, active counts by variance and
        by PCA eigenvalue."""
        active_units = [[1 if v > threshold else 0 for v in var] for var in variances]
        number_active_units = [int(sum(a)) for a in active_units]
        number_active_units_PCA = [int(sum(1 for e in eig if e > threshold)) for eig in eigen_values]
        return active_units, number_active_units, number_active_units_PCA

    def log_px_masked(self, x, masks, k=5000, eps=None):
        """Per-image k-sample log p(x) with every sampled h_i multiplied by
        masks[i] (0/1, length d_i) before log q and the later layers."""
        xd = self._x(x)
        N = xd.shape[0]
        L = len(self.n_latent_encoder)
        if len(masks) != L:
            raise ValueError(f"expected {L} masks, got {len(masks)}")
        with torch.cuda.stream(self._stream):
            mts = []
            for m, d in zip(masks, self.n_latent_encoder):
                t = torch.as_tensor(np.asarray(m, dtype=np.float32)).to(self.device).contiguous()
                if tuple(t.shape) != (d,):
                    raise ValueError(f"mask must have {d} entries, got {tuple(t.shape)}")
                mts.append(t)
            out = torch.empty(N, device=self.device)
        marr, nm = _lib.fptr_array(mts)
        arr, n, keep = self._eps(eps, N, k)
        self._call(self._lib.iwae_nll_masked(self._h, _lib.fptr(xd), N, int(k), arr, n, marr, nm, _lib.fptr(out)))
        self._stream.synchronize()
        return out

    def get_NLL_without_inactive_units(self, x, threshold=0.01, n_samples=5000, eps=None, eps_activity=None):
        """F:466-F:494: the activity of the units is measured on x with
        n_samples draws, inactive units are zeroed in every sample, and the
        n_samples-sample estimate is returned as -L_k (an NLL)."""
        variances, eigen_values = self.get_levels_of_units_activity(x, n_samples, eps_activity)
        active_units, _, _ = self.get_active_units(variances, eigen_values, threshold)
        return float(-self.log_px_masked(x, active_units, n_samples, eps).mean().item())

    def get_training_statistics(self, x, k, batch_size=10, batched=True, chunk_images=2000):
        """F:496-F:526: (res, res2) with the reference's keys.  res: batch
        means of VAE, IWAE, NLL (k=5000), E_q log p(x|h), both KL terms,
        reconstruction_loss, and LL_pruned (on the first batch); res2: active
        units (1000 draws over all of x), their counts, PCA counts, variances.

        batched=False runs the reference's loop literally: per batch of
        batch_size images (F:512) one launch series per statistic -- for 10k
        images, 2,000 k=5000 NLL calls of 10 images each (F:515, F:518).
        batched=True (default) evaluates each statistic over many batches per
        call (chunk_images, a multiple of batch_size; the k=5000 NLLs over all
        images at once, chunked by the library) and keeps the per-batch
        reduction: every statistic is a mean over images (equal batches), so
        the mean of the batch means is the chunk-size-weighted mean of the
        chunk means.  Each statistic still gets its own independent draw (the
        reference's separate get_L / get_NLL calls), per image."""
        xd = self._x(x)
        N = xd.shape[0]
        if batch_size <= 0 or N == 0 or N % batch_size != 0:
            # F:500 tf.reshape(x, (-1, batch_size, 28, 28, 1)) raises on a ragged tail
            raise ValueError(f"get_training_statistics: {N} images do not split into batches of {batch_size}")
        nb = N // batch_size
        res = dict(VAE=0.0, IWAE=0.0, NLL=0.0)
        res["E_q(h|x)[log(p(x|h))]"] = 0.0
        res["D_kl(q(h|x),p(h))"] = 0.0
        res["D_kl(q(h|x),p(h|x))"] = 0.0
        res["reconstruction_loss"] = 0.0
        if batched:
            step = max(batch_size, (int(chunk_images) // batch_size) * batch_size)
            for lo in range(0, N, step):
                b = xd[lo:lo + step]
                w = b.shape[0] / N                 # (its batches) / nb
                vae = self.get_L(b, k)
                res["VAE"] += vae * w
                res["IWAE"] += self.get_L_k(b, k) * w
                eq = self.get_E_qhIx_log_pxIh(b, k)
                res["E_q(h|x)[log(p(x|h))]"] += eq * w
                res["D_kl(q(h|x),p(h))"] += (eq - self.get_L(b, k)) * w
                res["D_kl(q(h|x),p(h|x))"] += -1 * self.get_L(b, k) * w
                res["reconstruction_loss"] += self.get_reconstruction_loss(b) * w
            nll1 = self.get_NLL(xd)                 # F:515, every batch in one launch series
            nll2 = self.get_NLL(xd)                 # F:518's second, independent estimate
            res["NLL"] = nll1
            res["D_kl(q(h|x),p(h|x))"] += -1 * nll2          # -(get_L + get_NLL), F:412
        else:
            for i in range(nb):
                b = xd[i * batch_size:(i + 1) * batch_size]
                vae = self.get_L(b, k)
                res["VAE"] += vae / nb
                res["IWAE"] += self.get_L_k(b, k) / nb
                res["NLL"] += self.get_NLL(b) / nb
                eq = self.get_E_qhIx_log_pxIh(b, k)
                res["E_q(h|x)[log(p(x|h))]"] += eq / nb
                res["D_kl(q(h|x),p(h))"] += (eq - self.get_L(b, k)) / nb
                res["D_kl(q(h|x),p(h|x))"] += -1 * (self.get_L(b, k) + self.get_NLL(b)) / nb
                res["reconstruction_loss"] += self.get_reconstruction_loss(b) / nb
        res2 = {}
        variances, eigen_values = self.get_levels_of_units_activity(xd, 1000)
        res2["active_units"], res2["number_of_active_units"], res2["number_of_PCA_active_units"] = \
            self.get_active_units(variances, eigen_values)
        res2["variances"] = variances
        res["LL_pruned"] = self.get_NLL_without_inactive_units(xd[:batch_size])
        return res, res2

    # ------------------------------------------------------------ data parallel
    def get_gradient_snr(self, x, k=None, R=1000, loss_function=None, p=None, alpha=None, beta=None, k1=None,
                         k2=None, seed=None, group=None):
        """Per-parameter gradient signal-to-noise ratio |E g| / std(g) over R
        independent noise draws at fixed weights (the
        estimator SNR of Rainforth et al. 2018, PDF p7).  Each draw is one
        device forward+backward (Philox noise, no Adam step); the moments
        sum g and sum g^2 accumulate on the device (iwae_grad_moments).  Under
        torch.distributed the R draws are split over the ranks (noise stream
        seed + rank) and the moments summed with one all-reduce each.
        Returns (list of SNR arrays in Keras weight order, {'R': R})."""
        from . import distributed as D
        rank, w = D.world(group)
        xd = self._x(x)
        B = xd.shape[0]
        lc = self._lc(loss_function, k, p, alpha, beta, k1, k2)
        if seed is not None:
            self._call(self._lib.iwae_set_seed(self._h, int(seed) & ((1 << 64) - 1)))
        if w > 1:
            self.set_noise_stream(rank)       # per-rank independent draws (also with the default seed)
        import ctypes
        g = _lib.FP()
        n = ctypes.c_longlong(0)
        self._call(self._lib.iwae_grad_buffer(self._h, ctypes.byref(g), ctypes.byref(n)))
        with torch.cuda.stream(self._stream):
            s1 = torch.zeros(int(n.value), device=self.device)
            s2 = torch.zeros(int(n.value), device=self.device)
        lo, hi = D.shard_range(int(R), rank, w)
        for _ in range(hi - lo):
            self._call(self._lib.iwae_forward_backward(self._h, lc, _lib.fptr(xd), B, None, 0,
                                                       _lib.fptr(self._loss_buf)))
            self._call(self._lib.iwae_grad_moments(self._h, _lib.fptr(s1), _lib.fptr(s2)))
        if w > 1:
            with torch.cuda.stream(self._stream):
                torch.distributed.all_reduce(s1, group=group)
                torch.distributed.all_reduce(s2, group=group)
        self._stream.synchronize()
        m1 = np.empty(self._nparams, np.float32)
        m2 = np.empty(self._nparams, np.float32)
        self._call(self._lib.iwae_export_internal(self._h, _lib.fptr(s1), m1.ctypes.data_as(_lib.FP), m1.size))
        self._call(self._lib.iwae_export_internal(self._h, _lib.fptr(s2), m2.ctypes.data_as(_lib.FP), m2.size))
        mean = m1.astype(np.float64) / R
        var = np.maximum(m2.astype(np.float64) / R - mean * mean, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            snr = np.where(var > 0, np.abs(mean) / np.sqrt(var), np.inf)
        return _split(snr, weight_shapes(self.dense)), {"R": int(R)}

    def _forward_backward(self, lc, xd, B, arr, n):
        self._call(self._lib.iwae_forward_backward(self._h, lc, _lib.fptr(xd), B, arr, n,
                                                   _lib.fptr(self._loss_buf)))

    def _apply_adam(self, scale):
        self._call(self._lib.iwae_apply_adam(self._h, float(scale)))


# ------------------------------------------------------------------ utils
def ctypes_stream(s):
    import ctypes
    return ctypes.c_void_p(int(s.cuda_stream))


def _split(flat, shapes):
    out, o = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(flat[o:o + n].reshape(s).copy())
        o += n
    assert o == flat.size
    return out


def _join(weights, shapes):
    if len(weights) != len(shapes):
        raise ValueError(f"expected {len(shapes)} weight arrays, got {len(weights)}")
    parts = []
    for w, s in zip(weights, shapes):
        a = np.asarray(w, np.float32)
        if a.shape != tuple(s):
            raise ValueError(f"weight of shape {a.shape} where {tuple(s)} is expected")
        parts.append(a.ravel())
    return np.ascontiguousarray(np.concatenate(parts), np.float32)
