"""Float64 restatement of the two inference entry points, with an error bound carried beside every value (numpy only;
the helpers at the end, which build the tests' nets, import torch and the package when called).

  student (lrl_ppo_act_student, actor_critic.py act_student):
      latent = adaptation_module(hist);  X = [obs | latent];  mean = actor_body(X)
  teacher (lrl_ppo_act with injected noise, ppo.py act):
      latent = env_factor_encoder(priv);  X = [obs | latent];  mu = actor_body(X);  values = critic_body(X)
      actions = mu + std * eps
      logp = sum_j (-z_j^2 / 2 - log std_j - log(2 pi) / 2),  z = (actions - mu) / std

Every MLP is x W^T + b per layer with ELU between the layers, written from these formulas (no torch module is called).
``params`` is the ActorCritic's state_dict as float64 arrays (``params_of``).

The bound.  An error travels as a pair: e, the elementwise bound [rows][width], and E, a bound on the 2-norm of each
row's error vector [rows].  Both are 0 on the call's inputs.  For one layer y = x W^T + b an fp32-class kernel's output
differs from the float64 y by at most

    e_out_i = min( sum_j |W_ij| e_j ,  ||W_i||_2 E )  +  u_i ,   u = EPS_PROD * (|x| |W|^T + |b|) + EPS_RND * |y|
    E_out   = min( sigma_max(W) E + ||u||_2 ,  ||e_out||_2 )

  * u is this layer's own error.  EPS_PROD = 1e-6 of sum |a b| per product is the project's own fp32-class bar for a
    GEMM of any family (tests/test_gemm_gpu.py::test_x6_error_is_fp32_class), here with the bias as one more term of
    the sum; EPS_RND = 2^-22 of |y| is the activation's and the store's roundings (four fp32 half-ulps).
  * The input's error d (|d_j| <= e_j, ||d||_2 <= E) comes out as W d.  Elementwise |W_i . d| <= sum_j |W_ij| e_j, and
    by Cauchy-Schwarz |W_i . d| <= ||W_i||_2 ||d||_2; as a vector ||W d||_2 <= sigma_max(W) ||d||_2 (the largest
    singular value, numpy's matrix 2-norm).  Every line is a worst case, none a statistical estimate.
  * ELU is 1-Lipschitz in every element, so it passes e unchanged and does not lengthen the error vector: E passes
    unchanged too.  |elu(y)| <= |y|, so the rounding term of the pre-activation covers the activated value.
  * X = [obs | latent]: e = [0 | e_latent], E = E_latent.

Why the pair.  The first form of this bound carried e alone, e_out = |W| e_in + u.  That lets every element's error
take the sign of its weight in every row of every layer at once, and the init_params nets' absolute row sums
(0.5 sqrt(fan_in): 11, 8, 5.6 in the bodies) compound: the latent's error reached the mean 600-fold, the mean's bound
was 30 % of the mean, and a bias dropped in the actor's last hidden layer or X's last float4 dropped from body 1 sat
below one bound.  The error vector cannot be aligned with all rows of W at once: its length grows by sigma_max(W)
(2.3, 1.0, 1.0 in the bodies) and only the last step to an element costs a row norm.  The same worst-case reasoning,
about 100 times tighter at the outputs; what it is relative to each output is printed by tests/test_act_ref.py.

The head (act_draw and act_head_kernel in csrc/lrl_ppo.hip).  The kernel forms act = fl(m + sd * e) from its own
fp32 mean m, then d = fl(act - m) and the term -(d d) / (2 sd sd) - logf(sd) - log sqrt(2 pi).  The error of m itself
cancels in d: what is left of z = d / sd against the exact z = e is the rounding of act (2^-24 |act|) and of the
subtraction, both inside dz_j = EPS_RND * (|mu_j| + |a_j|) / std_j.  To first order the term -z^2 / 2 moves by
|z_j| dz_j — the same first-order term as the formula's, so no other derivation is needed — and the squares, the
quotient, logf and the 12-term sum add roundings relative to the largest term: 12 * EPS_RND * max_j |term_j|.

    e_actions = e_mu + EPS_RND * (|mu| + |std * eps|)
    e_logp    = sum_j |z_j| dz_j + na * EPS_RND * max_j |term_j|          (na = 12 actions)

``student_eval`` / ``teacher_eval`` evaluate the same formulas, values only, in any dtype: in float32 they are the
plain fp32 evaluation that must stay inside the bound (tests/test_act_ref.py).
"""
import numpy as np

EPS_PROD = 1e-6       # tests/test_gemm_gpu.py::test_x6_error_is_fp32_class: |error| <= 1e-6 * sum |a b|
EPS_RND = 2.0 ** -22  # activation and store roundings

ACTOR, CRITIC, ENCODER, ADAPT = "actor_body", "critic_body", "env_factor_encoder", "adaptation_module"
NETS = ((42, 630), (48, 720), (235, 3525))  # (num_obs, num_hist): the presets', hist a multiple of 16, the perceptive
NUM_PRIV, NUM_ACTIONS = 18, 12


def params_of(ac):
    """The module's state_dict as float64 numpy arrays."""
    return {k: v.detach().double().cpu().numpy().copy() for k, v in ac.state_dict().items()}


def layers(params, prefix):
    """[(W, b)] of the Sequential ``prefix`` (Linear at the even indices, the activation between them)."""
    out, i = [], 0
    while f"{prefix}.{i}.weight" in params:
        out.append((params[f"{prefix}.{i}.weight"], params[f"{prefix}.{i}.bias"]))
        i += 2
    return out


def elu(y):
    return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))


_sigma = {}


def sigma_max(W):
    """The largest singular value of W (computed once per array)."""
    k = id(W)
    if k not in _sigma or _sigma[k][0] is not W:
        _sigma[k] = (W, float(np.linalg.norm(W, 2)))
    return _sigma[k][1]


def no_error(x):
    """The error pair (e, E) of an exact input."""
    return np.zeros(x.shape), np.zeros(x.shape[0])


def linear(x, W, b, err=None):
    """y = x W^T + b in x's dtype; with ``err`` (the input's error pair, float64) also the output's pair."""
    Wd, bd = W.astype(x.dtype), b.astype(x.dtype)
    y = x @ Wd.T + bd
    if err is None:
        return y
    e, E = err
    aW = np.abs(W)
    u = EPS_PROD * (np.abs(x) @ aW.T + np.abs(b)) + EPS_RND * np.abs(y)
    e_out = np.minimum(e @ aW.T, np.outer(E, np.linalg.norm(W, axis=1))) + u
    E_out = np.minimum(sigma_max(W) * E + np.linalg.norm(u, axis=1), np.linalg.norm(e_out, axis=1))
    return y, (e_out, E_out)


def mlp(params, prefix, x, err=None):
    """The MLP ``prefix`` over x: values (and, with ``err``, the error pair) of its last layer."""
    ls = layers(params, prefix)
    for i, (W, b) in enumerate(ls):
        if err is None:
            x = linear(x, W, b)
        else:
            x, err = linear(x, W, b, err)
        if i < len(ls) - 1:
            x = elu(x)
    return x if err is None else (x, err)


def with_obs(obs, latent, err):
    """X = [obs | latent] and its error pair."""
    return np.concatenate([obs, latent], -1), (np.concatenate([np.zeros_like(obs), err[0]], -1), err[1])


def head(mu, std, eps):
    """actions, logp, and the per-action z and terms."""
    std = std.astype(mu.dtype)
    actions = mu + std * eps
    z = (actions - mu) / std
    terms = -z * z / 2 - np.log(std) - mu.dtype.type(0.5 * np.log(2 * np.pi))
    return actions, terms.sum(-1), z, terms


def student_ref(params, obs, hist):
    """{mean, latent, bound_mean, bound_latent} of the student act in float64."""
    obs, hist = np.asarray(obs, np.float64), np.asarray(hist, np.float64)
    latent, err = mlp(params, ADAPT, hist, no_error(hist))
    X, eX = with_obs(obs, latent, err)
    mean, (e_mean, _) = mlp(params, ACTOR, X, eX)
    return {"mean": mean, "latent": latent, "bound_mean": e_mean, "bound_latent": err[0]}


def teacher_ref(params, obs, priv, eps):
    """{mu, actions, values, logp, bound_*} of the teacher act with injected noise in float64."""
    obs, priv, eps = (np.asarray(a, np.float64) for a in (obs, priv, eps))
    latent, err = mlp(params, ENCODER, priv, no_error(priv))
    X, eX = with_obs(obs, latent, err)
    mu, (e_mu, _) = mlp(params, ACTOR, X, eX)
    values, (e_v, _) = mlp(params, CRITIC, X, eX)
    std = params["std"]
    actions, logp, z, terms = head(mu, std, eps)
    e_act = e_mu + EPS_RND * (np.abs(mu) + np.abs(std * eps))
    dz = EPS_RND * (np.abs(mu) + np.abs(actions)) / std
    e_logp = (np.abs(z) * dz).sum(-1) + mu.shape[-1] * EPS_RND * np.abs(terms).max(-1)
    return {"mu": mu, "actions": actions, "values": values, "logp": logp, "bound_mu": e_mu, "bound_actions": e_act,
            "bound_values": e_v, "bound_logp": e_logp}


def student_eval(params, obs, hist, dtype=np.float32):
    obs, hist = np.asarray(obs, dtype), np.asarray(hist, dtype)
    latent = mlp(params, ADAPT, hist)
    return {"mean": mlp(params, ACTOR, np.concatenate([obs, latent], -1)), "latent": latent}


def teacher_eval(params, obs, priv, eps, dtype=np.float32):
    obs, priv, eps = (np.asarray(a, dtype) for a in (obs, priv, eps))
    X = np.concatenate([obs, mlp(params, ENCODER, priv)], -1)
    mu = mlp(params, ACTOR, X)
    actions, logp, _, _ = head(mu, params["std"], eps)
    return {"mu": mu, "actions": actions, "values": mlp(params, CRITIC, X), "logp": logp}


STUDENT_OUT = ("mean", "latent")
TEACHER_OUT = ("mu", "actions", "values", "logp")


def ratios(got, ref, names):
    """{output: worst |got - ref| / bound}; ``got`` values of any float dtype, shaped as the reference's or flat."""
    out = {}
    for k in names:
        r, b = ref[k], ref["bound_" + k]
        g = np.asarray(got[k], np.float64).reshape(r.shape)
        out[k] = float((np.abs(g - r) / b).max())
    return out


def inputs(num_obs, num_hist, n, seed=7):
    """obs, priv, hist, eps (float32, standard normal): the rows every accuracy test feeds, on the CPU and the GPU."""
    rng = np.random.default_rng([seed, num_obs, num_hist])
    return tuple(rng.standard_normal((n, k)).astype(np.float32) for k in (num_obs, NUM_PRIV, num_hist, NUM_ACTIONS))


# ---- the nets and rows of the act tests (torch and the package are imported on use) ----
def make_net(num_obs, num_hist):
    """The ActorCritic of the act tests: helpers.init_params, std = linspace(0.5, 1.5, 12)."""
    import torch
    from helpers import init_params
    from lrl.ppo.actor_critic import ActorCritic
    ac = ActorCritic(num_obs, NUM_PRIV, num_hist, NUM_ACTIONS)
    init_params(ac)
    with torch.no_grad():
        ac.std.copy_(torch.linspace(0.5, 1.5, NUM_ACTIONS))
    return ac


def trained_net():
    """(the trained checkpoint of tests/test_checkpoint.py as an ActorCritic, its fixture)"""
    import torch
    from helpers import golden
    from lrl.ppo.actor_critic import ActorCritic
    g = golden("checkpoint_last.npz")
    ac = ActorCritic(42, 18, 630, 12)
    ac.load_state_dict({k: torch.from_numpy(g["sd/" + k]) for k in g["keys"]}, strict=True)
    return ac, g


def trained_rows(g, n):
    """The checkpoint fixture's 64 rows cut (n < 64) or tiled (n > 64) to n, and noise for the teacher's head."""
    idx = np.arange(n) % 64
    eps = np.random.default_rng(5).standard_normal((n, NUM_ACTIONS)).astype(np.float32)
    return g["obs"][idx], g["priv"][idx], g["hist"][idx], eps
