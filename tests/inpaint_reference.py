"""The yardstick of the region-held sampler's tests: the reverse chain with positions held between the calls, composed on
the CPU from the oracle's pieces (oracle/diffsound_oracle.py: p_sample_step, q_sample, log_onehot, make_schedule) -- never
importing the package's sampler.  tools/make_inpaint_golden.py runs the same loops on the reference's own p_sample /
q_sample; tests/test_inpaint_host.py checks that the two agree token for token on every chain of the fixture.

    start state   [MASK] where free; where held: known (clamp) or a draw of q(x_{T-1} | x_0 = known) (renoise)
    call k        (t, t_post) = steps[k]:  x <- p_sample(x; t, posterior at t_post)  with uniforms noise_fn(k, shape),
                  then the held positions are overwritten: known (clamp, or t_post = 0), or a draw of
                  q(x_{t_post - 1} | x_0 = known) with uniforms hold_noise_fn(k + 1, shape)   (hold_noise_fn(0, .): the start)

Held positions are context of the denoiser and nothing else: the free positions of a call see exactly the arithmetic of
the unheld chain."""
import torch

import diffsound_oracle as O

L = 265


def chain_steps(num_timesteps, skip_step=0):
    """(t, t_post) per call: the plain chain, or sample_fast's (diffusion_transformer.py:790-804)"""
    if not skip_step:
        return [(s, s) for s in range(num_timesteps - 1, -1, -1)]
    lst = list(range(num_timesteps - 1, -1, -1 - skip_step))
    if lst[-1] != 0:
        lst.append(0)
    return [(s, s - skip_step if s > skip_step else s) for s in lst]


def inpaint_loop(sd, cond_emb, known, keep, noise_fn, num_timesteps=100, trunc_r=0.85, skip_step=0, mode="clamp",
                 hold_noise_fn=None, n_head=16, record=None):
    """known i64[B, L], keep bool[B, L] (True = held) -> tokens i64[B, L]; record: the tokens after every call."""
    assert mode in ("clamp", "renoise")
    K = sd["transformer.transformer.to_logits.1.weight"].shape[0]
    B = cond_emb.shape[0]
    shape = (B, K + 1, L)
    sched = O.make_schedule(num_timesteps, K + 1)
    log_known = O.log_onehot(known, K + 1)
    kp = keep[:, None, :]

    def held(t_out, call):       # the held positions' state at timestep t_out (< 0: clean)
        if mode == "clamp" or t_out < 0:
            return log_known
        return O.q_sample(sched, known, torch.full((B,), t_out, dtype=torch.long), hold_noise_fn(call, shape), K + 1)

    log_z = torch.where(kp, held(num_timesteps - 1, 0), O.initial_log_z(B, K + 1, L))
    for k, (s, sp) in enumerate(chain_steps(num_timesteps, skip_step)):
        t = torch.full((B,), s, dtype=torch.long)
        log_z = O.p_sample_step(sd, sched, log_z, cond_emb, t, noise_fn(k, shape), trunc_r, n_head,
                                t_post=torch.full((B,), sp, dtype=torch.long))
        log_z = torch.where(kp, held(sp - 1, k + 1), log_z)
        if record is not None:
            record.append(log_z.argmax(1).clone())
    return log_z.argmax(1)
