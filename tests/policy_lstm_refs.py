"""References for ouz_policy_rollout_lstm's tests: fixed weights of the recurrent actor and its f64
numpy restatement (the trunk, ``learner_refs.lstm_seq`` and ``learner_refs.policy_sample``)."""
import numpy as np

from tests import learner_refs as LR

LOGSTD = (-0.5, 0.0, 0.3, 1.0)
T1, T2, H = 512, 256, 128
NAMES = ("w1", "b1", "w2", "b2", "w_ih", "w_hh", "b_ih", "b_hh", "w_head", "b_head", "logstd")


def weights(seed=7):
    """(w1, b1, w2, b2, w_ih, w_hh, b_ih, b_hh, w_head, b_head, logstd) f32 numpy: random, every layer's
    pre-activations O(1) and O(1) head outputs (not the 0.01-std init, which would hide errors of what feeds it)."""
    g = np.random.default_rng(seed)
    f = np.float32
    return (f(g.standard_normal((T1, 13)) * 0.4), f(g.standard_normal(T1) * 0.1),
            f(g.standard_normal((T2, T1)) / np.sqrt(T1)), f(g.standard_normal(T2) * 0.1),
            f(g.standard_normal((4 * H, T2)) / np.sqrt(T2)), f(g.standard_normal((4 * H, H)) / np.sqrt(H)),
            f(g.standard_normal(4 * H) * 0.1), f(g.standard_normal(4 * H) * 0.1),
            f(g.standard_normal((4, H)) * 0.2), f(g.standard_normal(4) * 0.1), np.asarray(LOGSTD, f))


def actor64(w, x, done, h0, c0, eps, norm=None):
    """The recurrent actor over K steps in f64.  x (K, B, 13), done (K, B) (nonzero: the carry of the row is zeroed
    before the step), h0 / c0 (B, H), eps (K, B, 4).  Returns a dict: action (K, B, 4), logprob (K, B), hid (K, B, H),
    h_T / c_T (B, H): the carry after the last step, no done applied to it."""
    w1, b1, w2, b2, w_ih, w_hh, b_ih, b_hh, w_head, b_head, logstd = (np.asarray(t, np.float64) for t in w)
    x = np.asarray(x, np.float64)
    K, B, _ = x.shape
    if norm is not None:
        m, r, clip = norm
        x = np.clip((x - np.asarray(m, np.float64)) * np.asarray(r, np.float64), -clip, clip)
    feats = np.tanh(np.tanh(x.reshape(K * B, -1) @ w1.T + b1) @ w2.T + b2)
    x_proj = (feats @ w_ih.T + (b_ih + b_hh)).reshape(K, B, 4 * H)
    keep = 1.0 - (np.asarray(done) != 0).astype(np.float64)
    seq = LR.lstm_seq(x_proj, h0, c0, keep, w_hh)
    action, logprob, _ = LR.policy_sample(seq["hid"].reshape(K * B, H), w_head, b_head, logstd,
                                          np.asarray(eps, np.float64).reshape(K * B, 4))
    return {"action": action.reshape(K, B, 4), "logprob": logprob.reshape(K, B), "hid": seq["hid"],
            "h_T": seq["h_T"], "c_T": seq["c_T"]}


def load_actor(actor, w):
    """Copy ``weights()`` (numpy or torch) into a ``learners.models.LSTMActor``."""
    import torch
    t = [torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a) for a in w]
    with torch.no_grad():
        for dst, src in zip((actor.network[0].weight, actor.network[0].bias, actor.network[2].weight,
                             actor.network[2].bias, actor.lstm.weight_ih_l0, actor.lstm.weight_hh_l0,
                             actor.lstm.bias_ih_l0, actor.lstm.bias_hh_l0, actor.actor_mean.weight,
                             actor.actor_mean.bias), t[:10]):
            dst.copy_(src.to(dst.dtype))
        actor.actor_logstd.copy_(t[10].to(actor.actor_logstd.dtype).view(1, 4))
    return actor
