"""Numpy restatement of the device noise, written from csrc/iwae_kernels.h
(philox_normal4 / philox_normal2 / philox_uniform4), csrc/iwae_model.hip
(derive_key, the entry points' bases) and include/iwae.h (layer ids, rows).

The noise of one draw is a pure function of (key, base, row, layer, quad):
Philox4x32-10 on the counter (row, layer << 20 | quad, base_lo, base_hi) under
the key (key_lo, key_hi); the four words become float32 uniforms
u = ((float)c + 0.5f) * 2^-32 exactly as the kernel forms them, and Box-Muller
runs here in float64: columns 4g and 4g + 1 are sqrt(-2 ln u0) (cos, sin)(2 pi u1),
columns 4g + 2 and 4g + 3 the same from (u2, u3).  The integer part and the
uniforms are exact, so the only distance between the device's normals and these
is the device's v_log / v_sqrt / v_cos / v_sin rounding.

Philox itself, the uniform mapping and MAX_LAYERS are binarize_ref's (whose
Philox reproduces the published known answers, tests/test_binarize_ref.py)."""
import numpy as np

from binarize_ref import MAX_LAYERS, philox4x32_10, uniform_from_u32

MASK32 = 0xFFFFFFFF
MASK64 = (1 << 64) - 1

# Philox layer ids (include/iwae.h): encoder layer i draws under i ...
PIXEL_LAYER = 2 * MAX_LAYERS            # iwae_generate's pixel uniforms
SIR_LAYER = 2 * MAX_LAYERS + 1          # iwae_posterior / iwae_impute: the resampling uniform, value .x of quad 0
IMPUTE_LAYER = 2 * MAX_LAYERS + 2       # iwae_impute: the pixel uniforms of x_draw
BINARIZE_LAYER = 2 * MAX_LAYERS + 3     # iwae_binarize (binarize_ref.LAYER)


def prior_layer(j):
    """Prior layer j of the decoder (it samples h_{L-2-j}): iwae_generate's and iwae_reconstruct's."""
    return MAX_LAYERS + j


def top_layer(L):
    """h_L ~ N(0, I) of iwae_generate without h_top."""
    return MAX_LAYERS + L - 1


def splitmix64(z):
    z = (int(z) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def key(seed, stream=0):
    """derive_key (csrc/iwae_model.hip): the Philox key of noise stream `stream` under `seed`."""
    seed = int(seed) & MASK64
    stream = int(stream) & MASK64
    return seed if stream == 0 else splitmix64(seed ^ splitmix64(stream))


def words(key_, base, rows, quads, layer):
    """The four Philox words of every (row, quad): uint32 [4][len(rows)][len(quads)]."""
    rows = np.asarray(rows, np.uint64).reshape(-1, 1)
    quads = np.asarray(quads, np.uint64).reshape(1, -1)
    assert int(quads.max(initial=0)) < 1 << 20 and 0 <= int(layer) < 1 << 12
    shape = (rows.shape[0], quads.shape[1])
    c0 = np.broadcast_to(rows, shape)
    c1 = np.broadcast_to(np.uint64(int(layer) << 20) | quads, shape)
    c2 = np.full(shape, int(base) & MASK32, np.uint64)
    c3 = np.full(shape, (int(base) >> 32) & MASK32, np.uint64)
    return np.stack(philox4x32_10((c0, c1, c2, c3), (int(key_) & MASK32, (int(key_) >> 32) & MASK32)))


def box_muller(w, dtype=np.float64):
    """Words [4][...] -> normals [...][4] as philox_normal4 orders them.  The
    uniforms are the kernel's float32 ones; the logarithm, root, cosine and
    sine run in `dtype` (float32: a numpy evaluation, for scale only)."""
    u = [uniform_from_u32(c).astype(dtype) for c in w]
    two, tau = dtype(2.0), dtype(2.0 * np.pi)
    r0, r1 = np.sqrt(-two * np.log(u[0])), np.sqrt(-two * np.log(u[2]))
    return np.stack([r0 * np.cos(tau * u[1]), r0 * np.sin(tau * u[1]),
                     r1 * np.cos(tau * u[3]), r1 * np.sin(tau * u[3])], axis=-1)


def normals(key_, base, rows, d, layer, dtype=np.float64):
    """[len(rows), d]: the N(0, 1) noise of columns 0 .. d - 1 of the given rows."""
    rows = np.asarray(rows).ravel()
    ng = (int(d) + 3) // 4
    z = box_muller(words(key_, base, rows, np.arange(ng), layer), dtype)     # [rows, ng, 4]
    return z.reshape(len(rows), 4 * ng)[:, :d].copy()


def uniforms(key_, base, rows, d, layer):
    """[len(rows), d] float32: philox_uniform4's values, column j = value j % 4 of quad j / 4."""
    rows = np.asarray(rows).ravel()
    ng = (int(d) + 3) // 4
    w = words(key_, base, rows, np.arange(ng), layer)
    u = np.stack([uniform_from_u32(c) for c in w], axis=-1)
    return u.reshape(len(rows), 4 * ng)[:, :d].copy()


# ------------------------------------------------------------------ layouts
def sample_rows(B, k, first_image=0):
    """Rows of a forward pass in the oracle's [k][B] order: row = (first_image + b) k + s."""
    s, b = np.meshgrid(np.arange(k), np.arange(B), indexing="ij")
    return ((first_image + b) * k + s).ravel()


def eps_forward(key_, base, B, k, dims, first_image=0, dtype=np.float64):
    """The oracle's eps list [k][B][d_i] of one forward pass (train step, bound,
    log-weights, one NLL / posterior / encode chunk: rows local to the pass),
    encoder layer i under layer id i.  first_image = B: CIWAE's second draw,
    rows (B + b) k + s of the same pass."""
    rows = sample_rows(B, k, first_image)
    return [normals(key_, base, rows, d, i, dtype).reshape(k, B, d) for i, d in enumerate(dims)]


def eps_second_draw(key_, base, B, k, dims, dtype=np.float64):
    return eps_forward(key_, base, B, k, dims, first_image=B, dtype=dtype)


def eps_chunked(key_, base0, N, k, dims, imgs, ks=None):
    """eps [k][N][d_i] of a chunked pass (iwae_nll, iwae_posterior, iwae_impute,
    iwae_encode, iwae_encoder_means): image chunks of `imgs`, each in sample
    chunks of `ks` (default: all k); chunk c in call order draws at base0 + c
    with rows local to it (b_local * ks_local + s_local).  Returns (eps, the
    number of chunks = how far the call moves the position)."""
    ks = k if ks is None else ks
    out = [np.empty((k, N, d)) for d in dims]
    c = 0
    for i0 in range(0, N, imgs):
        n = min(imgs, N - i0)
        for s0 in range(0, k, ks):
            kl = min(ks, k - s0)
            for o, e in zip(out, eps_forward(key_, base0 + c, n, kl, dims)):
                o[s0:s0 + kl, i0:i0 + n] = e
            c += 1
    return out, c


def nll_chunks(N, k, chunk=0, nll_rows=1 << 20, nll_imgs=0):
    """nll_core's (images per chunk, samples per sample chunk)."""
    target = max(nll_rows, k)
    if chunk <= 0:
        chunk = nll_imgs
    imgs = min(chunk if chunk > 0 else max(1, target // k), N)
    return imgs, min(k, max(1, target // imgs))


def eps_prior(key_, base, n, dims):
    """iwae_generate's / iwae_reconstruct's prior draws in generation order:
    [1][n][d_{L-2-j}] under layer id MAX_LAYERS + j, row = the generated row."""
    L = len(dims)
    return [normals(key_, base, np.arange(n), dims[L - 2 - j], prior_layer(j))[None] for j in range(L - 1)]


def eps_top(key_, base, n, dims):
    """h_L of iwae_generate without h_top: [1][n][d_L]."""
    return normals(key_, base, np.arange(n), dims[-1], top_layer(len(dims)))[None]


def pixel_uniforms(key_, base, n, x_dim, layer=PIXEL_LAYER):
    return uniforms(key_, base, np.arange(n), x_dim, layer)


def sir_uniforms(key_, base0, N, imgs):
    """[N] float32: the resampling uniform of image b, row = its index in its
    chunk, the chunk's base (the one its first pass drew with)."""
    out = np.empty(N, np.float32)
    for c, i0 in enumerate(range(0, N, imgs)):
        n = min(imgs, N - i0)
        out[i0:i0 + n] = uniforms(key_, base0 + c, np.arange(n), 1, SIR_LAYER)[:, 0]
    return out


def impute_uniforms(key_, base0, N, x_dim, imgs):
    out = np.empty((N, x_dim), np.float32)
    for c, i0 in enumerate(range(0, N, imgs)):
        n = min(imgs, N - i0)
        out[i0:i0 + n] = uniforms(key_, base0 + c, np.arange(n), x_dim, IMPUTE_LAYER)
    return out


# ---------------------------------------------------- how far a call moves
def _ceil(a, b):
    return -(-a // b)


def _nll_advance(N, k, chunk=0, nll_rows=1 << 20, nll_imgs=0):
    imgs, ks = nll_chunks(N, k, chunk, nll_rows, nll_imgs)
    return _ceil(N, imgs) * _ceil(k, ks)


def _image_chunks(N, k, chunk=0, nll_rows=1 << 20, nll_imgs=0):
    """iwae_posterior / iwae_impute / iwae_score / iwae_encode: a chunk holds all k samples."""
    if chunk <= 0:
        chunk = nll_imgs
    imgs = min(chunk if chunk > 0 else max(1, nll_rows // k), N)
    return _ceil(N, imgs)


# entry point: advances of the noise position, restated from csrc/iwae_model.hip
# (who advances: bound_kernel / the engine's in-launch bound for a forward pass,
# launch_lse per NLL launch, group_mean's last layer, gen_kernel's last workgroup
# or launch_rng_advance)
ADVANCE = {
    "train_step": lambda **a: 1,                        # one forward pass (CIWAE's two draws share it)
    "train_steps": lambda nsteps, **a: nsteps,
    "forward_backward": lambda **a: 1,
    "bound": lambda **a: 1,
    "log_weights": lambda **a: 1,
    "e_log_px": lambda **a: 1,
    "nll": _nll_advance,                                # one per (image chunk, sample chunk)
    "nll_partials": _nll_advance,
    "encoder_means": lambda N, n, **a: _ceil(N, min(N, max(1, (1 << 20) // n))),
    "posterior": _image_chunks,
    "impute": _image_chunks,
    "encode": _image_chunks,
    "generate": lambda n, **a: 1 if n > 0 else 0,
    "reconstruct": lambda **a: 1,
    "binarize": lambda n, **a: 1 if n > 0 else 0,
    "score": lambda **a: 0,
}


def advance(entry, **args):
    return ADVANCE[entry](**args)


# ------------------------------------------------------------------- cases
# The inputs tests/test_noise_ref.py (CPU) and tests/test_gpu_noise.py share: the
# small models of sample_cases (x_dim = 20), one two-layer model whose latent
# widths are off 4 and above 64 (a lane-strided quad loop runs twice, the last
# quad is partly used, philox_normal2's odd half lands on the last column), and
# test_gpu_state's weight-ring architecture for the points only it can reach.
SEED = 0xC0FFEE1234567891          # both key words in use
X_DIM = 20
MODELS = {"S1": ([24], [6]), "S2": ([20, 12], [6, 4]), "W2": ([48, 32], [70, 5])}
RING_ARCH = ([200, 100], [100, 200], [100, 50], [100, 784])
SHAPES = ((3, 17), (5, 1))          # an image straddles a 16-row tile; one sample per image
PARAM_SEED = {"S1": 1501, "S2": 1502, "W2": 1503, "RING": 1504}
TRAIN_LOSSES = ("VAE", "IWAE", "CIWAE", "PIWAE", "IWAE_DREG")
TRAIN_PATHS = ("layerwise", "fused", "auto")
# (model, B, k, loss id): every loss on the two-layer models at both shapes, IWAE on S1,
# PIWAE with a split that is not trivial (k = 18 = 6 * 3)
TRAIN = [(m, B, k, v) for m in ("S2", "W2") for B, k in SHAPES for v in TRAIN_LOSSES] + \
        [("S1", B, k, "IWAE") for B, k in SHAPES] + [("S2", 3, 18, "PIWAE")]
RING_POINT = ("RING", 17, 241, "IWAE")      # 4097 sample rows: wide engine launches, weight-ring forward / backward
STEPS = ("S2", 3, 17, 3)                    # three consecutive steps on 3 * B images
FORWARD = [(m, B, k) for m in MODELS for B, k in SHAPES]
NLL_N = 5


def arch(model):
    import shape_cases as S
    if model == "RING":
        return RING_ARCH, RING_ARCH[3][-1]
    he, le = MODELS[model]
    hd, ld = S._mirror(he, le, X_DIM)
    return (list(he), hd, list(le), ld), X_DIM


_CACHE = {}


def case(model, B):
    """(architecture, spec, params, mean, x [B, x_dim]) in float64, the parameters
    rounded through float32 (pathgrad_ref.make_case).  Shared: do not modify."""
    import pathgrad_ref as R
    if (model, B) not in _CACHE:
        a, x_dim = arch(model)
        spec, params, mean, x, _ = R.make_case(a, B, 1, PARAM_SEED[model], x_dim=x_dim)
        x.setflags(write=False)
        _CACHE[model, B] = (a, spec, params, mean, x)
    return _CACHE[model, B]


def loss_kw(vid, k):
    if vid == "CIWAE":
        return dict(beta=0.3)
    if vid == "PIWAE":
        return dict(k1=6, k2=3) if k == 18 else dict(k1=k, k2=1)
    return {}


def oracle_step(params, spec, x, k, vid, base, opt, dtype=np.float64, key_=None):
    """One oracle train step on the reference noise of position `base`:
    (loss, new parameters, flat gradient)."""
    import pathgrad_ref as R
    from oracle import iwae_oracle as O
    key_ = key(SEED) if key_ is None else key_
    B, dims = x.shape[0], spec.n_latent_encoder
    eps = [e.astype(dtype) for e in eps_forward(key_, base, B, k, dims)]
    p = O.cast_params(params, dtype)
    if vid in R.LOSSES:
        return R.train_step(p, spec, x.astype(dtype), eps, vid, opt)
    kw = loss_kw(vid, k)
    if vid == "CIWAE":
        kw["eps2"] = [e.astype(dtype) for e in eps_second_draw(key_, base, B, k, dims)]
    return O.train_step(p, spec, x.astype(dtype), eps, vid, k, opt, **kw)


def train_reference(model, B, k, vid, dtype=np.float64):
    """(loss, flat gradient, flat post-Adam weights) of the first train step after
    set_seed(SEED) (Adam lr 1e-3, eps 1e-4), by the oracle in `dtype` arithmetic."""
    from oracle import iwae_oracle as O
    ck = ("train", model, B, k, vid, np.dtype(dtype).name)
    if ck not in _CACHE:
        _, spec, params, _, x = case(model, B)
        out = oracle_step(params, spec, x, k, vid, 0, O.Adam(1e-3, 0.9, 0.999, 1e-4), dtype)
        res = (float(out[0]), np.asarray(out[2], np.float64), np.asarray(O.flatten_params(spec, out[1]), np.float64))
        for a in res[1:]:
            a.setflags(write=False)
        _CACHE[ck] = res
    return _CACHE[ck]


def steps_reference(dtype=np.float64):
    """STEPS through Adam: step i on batch i with the noise of position i;
    (losses, final flat weights)."""
    from oracle import iwae_oracle as O
    ck = ("steps", np.dtype(dtype).name)
    if ck not in _CACHE:
        model, B, k, n = STEPS
        _, spec, params, _, _ = case(model, B)
        xs = steps_images()
        opt = O.Adam(1e-3, 0.9, 0.999, 1e-4)
        losses = []
        for i in range(n):
            loss, params, _ = oracle_step(params, spec, xs[i * B:(i + 1) * B], k, "IWAE", i, opt, dtype)
            losses.append(float(loss))
        _CACHE[ck] = (np.asarray(losses), np.asarray(O.flatten_params(spec, params), np.float64))
    return _CACHE[ck]


def steps_images():
    model, B, k, n = STEPS
    mean = case(model, B)[3]
    return (np.random.default_rng(1601).random((n * B, X_DIM)) < mean).astype(np.float64)


def forward_reference(model, B, k, base=0, dtype=np.float64, key_=None):
    """The oracle's forward cache on the reference noise of one pass at `base`."""
    from oracle import iwae_oracle as O
    key_ = key(SEED) if key_ is None else key_
    _, spec, params, _, x = case(model, B)
    eps = [e.astype(dtype) for e in eps_forward(key_, base, B, k, spec.n_latent_encoder)]
    return O.forward(O.cast_params(params, dtype), spec, x.astype(dtype), eps, need_bce=True)


# log p(x): (model, N, k, chunk argument, nll_rows knob or None).  N = 5 in image
# chunks of 2; nll_rows below imgs * k splits a chunk's samples (S2 / W2: 17 ->
# 8 + 8 + 1; RING: 130 -> 128 on the weight ring + 2 on mega_fwd_kernel)
NLL = [("S2", NLL_N, 17, 2, None), ("S2", NLL_N, 17, 2, 16), ("W2", NLL_N, 17, 2, 16), ("S1", NLL_N, 17, 2, 16),
       ("RING", NLL_N, 130, 2, None), ("RING", NLL_N, 130, 2, 256)]
NLL_MASKED = ("S2", NLL_N, 17, 16)           # log_px_masked: (model, N, k, nll_rows)
STAT_MODELS = ("S2", "W2")
# (W2's 70 latent units spread an image's 17 Glorot-weight log-weights over more than 80 nats: its
# smallest normalised weights leave float32's normal range, and the weights' bars need log w~)
POSTERIOR_MODELS = ("S1", "S2")
POSTERIOR_K = 17
MEANS_N = 8


def latent_masks(model):
    """0/1 unit masks of log_px_masked: every third unit off."""
    dims = arch(model)[0][2]
    return [(np.arange(d) % 3 != 1).astype(np.float64) for d in dims]


def nll_reference(model, N, k, chunk, nll_rows=None, base=0, dtype=np.float64, masks=None):
    """(log p(x) [N], chunks) of a chunked NLL that starts at `base`."""
    from oracle import iwae_oracle as O
    ck = ("nll", model, N, k, chunk, nll_rows, base, np.dtype(dtype).name, masks is not None)
    if ck not in _CACHE:
        _, spec, params, _, x = case(model, N)
        imgs, ks = nll_chunks(N, k, chunk, **({} if nll_rows is None else dict(nll_rows=nll_rows)))
        eps, chunks = eps_chunked(key(SEED), base, N, k, spec.n_latent_encoder, imgs, ks)
        eps = [e.astype(dtype) for e in eps]
        lp = O.log_px_per_image(O.cast_params(params, dtype), spec, x.astype(dtype), k, eps=eps,
                                masks=None if masks is None else [m.astype(dtype) for m in masks])
        _CACHE[ck] = (np.asarray(lp, np.float64), chunks)
    return _CACHE[ck]


def reconstruct_reference(model, B, base=0, dtype=np.float64):
    """(probs [B, x_dim], loss): encoder ids 0 .. L - 1 at row b, then the prior ids, one base."""
    from oracle import iwae_oracle as O
    _, spec, params, _, x = case(model, B)
    dims = spec.n_latent_encoder
    e_enc = [e.astype(dtype) for e in eps_forward(key(SEED), base, B, 1, dims)]
    e_pri = [e.astype(dtype) for e in eps_prior(key(SEED), base, B, dims)]
    return O.reconstruct(O.cast_params(params, dtype), spec, x.astype(dtype), e_enc, e_pri)


def encoder_means_reference(model, N, n, base=0, dtype=np.float64):
    from oracle import iwae_oracle as O
    _, spec, params, _, x = case(model, N)
    eps = [e.astype(dtype) for e in eps_forward(key(SEED), base, N, n, spec.n_latent_encoder)]
    return O.encoder_means(O.cast_params(params, dtype), spec, x.astype(dtype), eps)


def generate_reference(model, n, base=0, dtype=np.float64):
    """Decoder.generate_x (F:107-F:119) on the reference noise of position `base`:
    (probs [n, x_dim], latents h_1 .. h_L, the pixel uniforms [n, x_dim])."""
    from oracle import iwae_oracle as O
    _, spec, params, _, _ = case(model, SHAPES[0][0])
    p = O.cast_params(params, dtype)
    dims = spec.n_latent_encoder
    hs = [eps_top(key(SEED), base, n, dims)[0].astype(dtype)]
    for j, e in enumerate(eps_prior(key(SEED), base, n, dims)):
        dj = O._stoch_forward(p, f"dec{j}", hs[-1])
        hs.append(e[0].astype(dtype) * dj["scale"] + dj["mu"])
    (W1, b1), (W2, b2), (W3, b3) = p["out.l1"], p["out.l2"], p["out.l3"]
    logit = np.tanh(np.tanh(hs[-1] @ W1 + b1) @ W2 + b2) @ W3 + b3
    probs = (1 / (1 + np.exp(-logit))) * dtype(O.PROB_SCALE) + dtype(O.PROB_SHIFT)
    return probs, hs[::-1], pixel_uniforms(key(SEED), base, n, spec.x_dim)


def pixel_mask(N, x_dim):
    """Observed-pixel mask of the imputation case: image 0 complete, image 1
    all missing, the others half observed."""
    mask = (np.random.default_rng(1603).random((N, x_dim)) < 0.5).astype(np.float32)
    mask[0], mask[1] = 1.0, 0.0
    return mask


def posterior_reference(model, N, k, imgs, base=0, mask=None):
    """tests/posterior_ref.py (or impute_ref.py with `mask`) on the reference
    noise: chunks of `imgs` images from `base`, the resampling uniform and the
    imputation's pixel uniforms of each chunk's base."""
    import impute_ref as I
    import posterior_ref as P
    ck = ("post", model, N, k, imgs, base, mask is not None)
    if ck not in _CACHE:
        _, spec, params, _, x = case(model, N)
        eps, chunks = eps_chunked(key(SEED), base, N, k, spec.n_latent_encoder, imgs)
        u = sir_uniforms(key(SEED), base, N, imgs)
        if mask is None:
            ref = P.posterior(params, spec, x, eps, u)
        else:
            ref = I.impute(params, spec, x, mask, eps, u, impute_uniforms(key(SEED), base, N, spec.x_dim, imgs))
        ref.update(u=u, eps=eps, chunks=chunks)
        _CACHE[ck] = ref
    return _CACHE[ck]
