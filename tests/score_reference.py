"""The yardstick of likelihood scoring: one term of the variational bound per row, restated from the
oracle's own pieces -- diffsound_oracle.make_schedule / predict_start / q_posterior, the functions the sampling and training
goldens validate -- in the dtype the caller names.  float64 is the yardstick; float32 is the same restatement in the kernels'
working precision, and its distance from float64 (d32) is the unit the GPU tests' tolerances are stated in.  Host only."""
import torch

import diffsound_oracle as O


def schedule(K, T, dtype):
    """the fp32 schedule buffers of the model, taken to dtype (oracle train_loss does the same)"""
    return {k: v.to(dtype) for k, v in O.make_schedule(T, K + 1).items()}


def score_terms(logits, x0, xt, t, T, dtype):
    """logits f32[B, K, L] (the network's output on (xt, t)), x0 / xt i64[B, L], t i64[B] in [0, T) ->
    (pos dtype[B, L], term f64[B]): per position the decoder NLL -log p(x0 | x1) where t == 0 and
    KL(q(x_{t-1} | x_t, x0) || p(x_{t-1} | x_t)) where t > 0 (diffusion_transformer.py:439-446 with mask weights (1, 1));
    per row their sum, the positions widened to double first."""
    K = logits.shape[1]
    sched = schedule(K, T, dtype)
    log_x0 = O.log_onehot(x0, K + 1).to(dtype)
    log_xt = O.log_onehot(xt, K + 1).to(dtype)
    recon = O.predict_start(logits, dtype)
    model = O.q_posterior(sched, recon, log_xt, t)
    true = O.q_posterior(sched, log_x0, log_xt, t)
    kl = (true.exp() * (true - model)).sum(1)
    nll = -(log_x0.exp() * model).sum(1)
    pos = torch.where((t == 0)[:, None], nll, kl)
    return pos, pos.double().sum(-1)


def forward_terms(sd, x0, xt, cond, t, T, n_head=16):
    """The same with the oracle's own network in the dtype of the state dict sd: logits = transformer_forward(sd, xt, cond, t).
    -> (pos, term f64[B])"""
    dtype = sd["transformer.transformer.to_logits.1.weight"].dtype
    logits = O.transformer_forward(sd, xt, cond.to(dtype), t, n_head=n_head)
    return score_terms(logits, x0, xt, t, T, dtype)
