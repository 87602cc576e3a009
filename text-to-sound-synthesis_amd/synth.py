"""Seeded synthetic weights and inputs, keyed by state-dict name.

The reference ships no checkpoints, so parity and bench runs use
random weights with the reference's exact shapes.  Values depend only on
(seed, state-dict key, shape) -- never on construction order -- so the same
tensors can be poured into the reference modules (oracle/make_golden.py, run
in the build container), into the CPU oracle and into the HIP
modules on the GPU box, without the reference being present there.

Distributions follow the reference initialisers in spirit
(transformer_utils.py:355-363 N(0,0.02); conv default ~U(+-1/sqrt(fan_in));
quantize.py:24 U(+-1/K)), but biases and norm affines are made non-trivial so
that every term of every kernel is exercised.
"""
import zlib

import torch


def _gen(seed, key):
    g = torch.Generator(device="cpu")
    g.manual_seed((zlib.crc32(key.encode()) ^ (seed * 0x9E3779B1)) & 0x7FFFFFFF)
    return g


def synth_tensor(key, shape, seed=0, dtype=torch.float32):
    """One deterministic tensor for a state-dict entry."""
    g = _gen(seed, key)
    shape = tuple(shape)
    leaf = key.rsplit(".", 1)[-1]
    nd = len(shape)
    if key.endswith("quantize.embedding.weight"):
        k = shape[0]
        t = (torch.rand(shape, generator=g) * 2 - 1) / k
    elif leaf == "bias":
        t = torch.randn(shape, generator=g) * 0.02
    elif leaf == "weight_g":
        # filled in by synth_state_dict from the sibling weight_v
        t = torch.randn(shape, generator=g)
    elif nd == 1:  # norm scale
        t = 1.0 + 0.1 * torch.randn(shape, generator=g)
    elif nd == 2:  # Linear / Embedding of the transformer
        t = torch.randn(shape, generator=g) * 0.02
    else:  # conv kernels: [out, in, k...] (or [in, out, k] transposed)
        fan_in = 1
        for s in shape[1:]:
            fan_in *= s
        t = torch.randn(shape, generator=g) * (1.0 / (3.0 * fan_in) ** 0.5)
        if leaf == "weight_v":
            t = t * 3.0 ** 0.5
    return t.to(dtype)


# ---- "trained-like" statistics for the denoiser (profile="trained") ---------------------------------------------------
# Every other vector in tests/golden comes from N(0, 0.02) initialiser-like weights: activations are O(1), LayerNorm
# gains are 1 +- 0.1, nothing comes near fp16's range.  Trained transformers do not look like that: LayerNorm / AdaLN
# gains spread over decades, a handful of hidden channels carry activations ~100x the rest, weight matrices are
# heavy-tailed, and single rows drive an activation towards the top of the fp16 range.  This profile synthesises those
# features (no checkpoint exists) so that the split-fp16 arithmetic -- per-matrix power-of-two
# weight scale, un-scaled activations saturating at 65504 -- meets the reference off the initialiser manifold.
OUTLIER_CHANNELS = (17, 300, 511, 900)      # hidden channels of the residual stream that run ~100x hot


def _trained_tensor(key, shape, seed):
    g = _gen(seed, "trained:" + key)
    shape = tuple(shape)
    leaf = key.rsplit(".", 1)[-1]
    nd = len(shape)
    if nd == 2 and leaf == "weight":
        # heavy tails: Student-t with 3 degrees of freedom, scaled to the initialiser's standard deviation
        z = torch.randn(shape, generator=g)
        chi = (torch.randn((3,) + shape, generator=g) ** 2).sum(0) / 3.0
        t = 0.02 * z / chi.sqrt() / 3.0 ** 0.5
        if ".emb." in key or key.endswith("_emb.weight"):
            t = 0.02 * z                       # embedding tables stay Gaussian ...
            if key.endswith("content_emb.emb.weight"):
                t[:, list(OUTLIER_CHANNELS)] *= 100.0          # ... the token table with hot residual-stream channels
        elif key.endswith(("attn1.proj.weight", "attn2.proj.weight", "mlp.2.weight")):
            t[list(OUTLIER_CHANNELS), :] *= 8.0                # the blocks keep writing into the hot channels
        elif key.endswith("mlp.0.weight"):
            t[5, :] *= 2000.0                                   # one hidden unit whose activation runs into the 1e4s (fp16 tops out at 65504)
        elif key.endswith(("ln1.linear.weight", "ln1_1.linear.weight")):
            t = t * 4.0                                         # AdaLN scale / shift with real dynamic range
        return t
    if nd == 1 and leaf == "weight":                            # LayerNorm gains: log-uniform over 0.1 .. 10
        return 10.0 ** (torch.rand(shape, generator=g) * 2.0 - 1.0)
    if leaf == "bias":
        return torch.randn(shape, generator=g) * 0.1
    return None


# ---- "trained-like" statistics for the codec and the vocoder (profile="trained_conv") -----------------------------------
# The split-fp16 convolutions of the SpecVQGAN codec and the MelGAN vocoder split UN-normalised fp32 activations: the split is
# fp32-class only for |a| in about [2^-3, 65504].  This profile pushes both networks to the two edges of that band: GroupNorm
# gains over two decades, Student-t conv weights, residual streams whose hot channels grow level by level to ~2^14 (below
# 65504) in front of the decoder's upsample convs and the encoder's stride-2 convs, a codebook with O(1) norms and near-duplicate
# codes, MelGAN weight_g over a decade and a last vocoder stage whose every split operand stays below 2^-3.
CODEC_HOT = (3, 77)                         # stream channels that run hot (exist at every width: 128 .. 512)
CODEC_HOT_GAIN = {"decoder": (200.0, 2400.0, 2400.0, 2400.0, 3600.0), "encoder": (2000.0, 1700.0, 2200.0, 2300.0, 6.0)}  # conv2 rows
MELGAN_QUIET = ("model.18.", "model.19.", "model.20.", "model.21.")   # the last stage: ConvTranspose1d 64 -> 32 + its 3 blocks
MELGAN_QUIET_GAIN = (4e-5, 0.4)          # weight_g factor of its ConvTranspose1d / of its blocks' convs


def _student_t(g, shape, std):
    z = torch.randn(shape, generator=g)
    chi = (torch.randn((3,) + tuple(shape), generator=g) ** 2).sum(0) / 3.0
    return std * z / chi.sqrt() / 3.0 ** 0.5


def _trained_conv_tensor(key, shape, seed):
    g = _gen(seed, "trained_conv:" + key)
    shape = tuple(shape)
    leaf = key.rsplit(".", 1)[-1]
    nd = len(shape)
    if key.endswith("quantize.embedding.weight"):
        # O(1) norms; codes 2j + 1 (j < 8) are near-duplicates of codes 2j, so the code search meets argmin near-ties
        t = torch.randn(shape, generator=g) / shape[1] ** 0.5
        t[1:16:2] = t[0:16:2] + 1e-3 * torch.randn((8, shape[1]), generator=g) / shape[1] ** 0.5
        return t
    if key.startswith("content_codec."):
        if nd == 1 and leaf == "weight":                         # GroupNorm gains: log-uniform over 0.1 .. 10
            return 10.0 ** (torch.rand(shape, generator=g) * 2.0 - 1.0)
        if leaf == "bias":
            return torch.randn(shape, generator=g) * 0.1
        if nd == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            t = _student_t(g, shape, 1.0 / (3.0 * fan_in) ** 0.5)
            part = key.split(".")[1]
            if key.endswith("conv2.weight") and ".block." in key and part in CODEC_HOT_GAIN:
                # the residual branches keep writing into the hot channels: the stream grows level by level
                lvl = int(key.split(".up." if part == "decoder" else ".down.")[1].split(".")[0])
                t[list(CODEC_HOT)] *= CODEC_HOT_GAIN[part][lvl]
            elif key.endswith("nin_shortcut.weight"):
                for c in CODEC_HOT:                              # the hot channels survive a change of width
                    t[c, c] = 1.0
            return t
        return None
    if key.startswith("model."):
        quiet = key.startswith(MELGAN_QUIET)
        if leaf == "weight_v":
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            return _student_t(g, shape, 1.0 / fan_in ** 0.5)
        if leaf == "weight_g":                                   # a factor over a decade around ||v|| (applied below)
            f = 10.0 ** (torch.rand(shape, generator=g) - 0.5)
            if quiet:
                f = f * MELGAN_QUIET_GAIN[int(".block." in key or ".shortcut." in key)]
            return f
        if leaf == "bias":
            return torch.randn(shape, generator=g) * (0.002 if quiet else 0.05)
    return None


# ---- "trained-like" statistics for the CLIP text tower (profile="trained_clip") ------------------------------------------
# The tower runs in fp16 semantics: every op's output is rounded to the fp16 grid.  At init its attention scores stay below 9
# and its activations are O(1), so that rounding is at its mildest.  This profile starts from the init tensor of each key and
# gives it what a trained text tower has: LayerNorm gains spread over a decade, three hot residual channels fed by the token
# table and kept hot by the blocks' output projections, and query / key projections large enough for sharply peaked causal
# attention (scores in the 30s to 40s on the golden captions).
CLIP_PREFIX = "transformer.condition_emb."
CLIP_HOT = (31, 255, 480)                    # residual channels of the 512-wide text tower that run hot


def _trained_clip_tensor(key, shape, seed):
    if not key.startswith(CLIP_PREFIX):
        return None
    name = key[len(CLIP_PREFIX):]
    if name.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):     # log-uniform over 10^-0.5 .. 10^0.5
        return 10.0 ** (torch.rand(tuple(shape), generator=_gen(seed, "trained_clip:" + key)) - 0.5)
    if name == "token_embedding.weight":
        t = synth_tensor(key, shape, seed)
        t[:, list(CLIP_HOT)] *= 50.0
        return t
    if name.endswith("attn.in_proj_weight"):
        t = synth_tensor(key, shape, seed)
        t[:2 * shape[1]] *= 4.0                                                # the query and the key rows
        return t
    if name.endswith(("attn.out_proj.weight", "mlp.c_proj.weight")):
        t = synth_tensor(key, shape, seed)
        t[list(CLIP_HOT)] *= 8.0                                               # the blocks keep writing into the hot channels
        return t
    return None


def synth_state_dict(shapes, seed=0, profile="init"):
    """shapes: {key: shape}.  Returns {key: tensor}; weight_g follows weight_v.  profile = "trained": the denoiser's
    tensors (keys under transformer.transformer.) get trained-like statistics, see above; profile = "trained_conv": the
    codec's (content_codec.*) and the vocoder's (model.*) tensors do; profile = "trained_clip": the text tower's
    (transformer.condition_emb.*) do; everything else as "init"."""
    if profile not in ("init", "trained", "trained_conv", "trained_clip"):
        raise ValueError("unknown profile %r" % (profile,))
    out = {}
    factor_g = set()
    for k, shp in shapes.items():
        t = None
        if profile == "trained" and (k.startswith("transformer.transformer.") or k.startswith("transformer.blocks.")
                                     or k.startswith("blocks.")):
            t = _trained_tensor(k, shp, seed)
        elif profile == "trained_conv":
            t = _trained_conv_tensor(k, shp, seed)
            if t is not None and k.endswith("weight_g"):
                factor_g.add(k)
        elif profile == "trained_clip":
            t = _trained_clip_tensor(k, shp, seed)
        out[k] = synth_tensor(k, shp, seed) if t is None else t
    for k in list(out):
        if k.endswith("weight_g"):
            v = out.get(k[:-1] + "v")
            if v is not None:
                # torch weight_norm: norm over all dims except 0 (vocoder/modules.py:18-23)
                nrm = v.reshape(v.shape[0], -1).norm(dim=1).reshape(out[k].shape)
                out[k] = nrm * out[k] if k in factor_g else nrm * (1.0 + 0.1 * out[k])
    return out


@torch.no_grad()
def synth_init_(module, seed=0, prefix="", skip=(), profile="init"):
    """Fill every parameter of `module` from its state-dict key (in place).

    Floating-point buffers are left alone (schedules etc. are computed, not random)."""
    shapes = {prefix + n: tuple(p.shape) for n, p in module.named_parameters()
              if not any(n.startswith(s) for s in skip)}
    sd = synth_state_dict(shapes, seed, profile)
    for n, p in module.named_parameters():
        k = prefix + n
        if k in sd:
            p.copy_(sd[k].to(p.dtype))
    return module


def synth_tokens(batch, length=265, num_codes=256, mask_frac=0.3, seed=0, key="tokens"):
    """Token grid with a controllable share of [MASK] (= num_codes)."""
    g = _gen(seed, key)
    tok = torch.randint(0, num_codes, (batch, length), generator=g)
    m = torch.rand((batch, length), generator=g) < mask_frac
    tok[m] = num_codes
    return tok.long()


def synth_cond_emb(batch, seq=77, dim=512, seed=0, key="cond_emb"):
    """Stand-in for CLIPTextEmbedding output: rows L2-normalised
    (clip_text_embedding.py:79-80)."""
    g = _gen(seed, key)
    x = torch.randn((batch, seq, dim), generator=g)
    return x / x.norm(dim=-1, keepdim=True)


def synth_uniform(shape, seed=0, key="u"):
    g = _gen(seed, key)
    return torch.rand(tuple(shape), generator=g)


_WORDS = ("a dog barks while birds chirp in the distance rain falls on metal roof "
          "engine idles then revs people talk and laugh water flows wind blows "
          "door slams glass breaks music plays softly crowd cheers siren wails "
          "keyboard typing footsteps on gravel thunder rumbles cat meows baby cries "
          "bell rings train passes helicopter hovers waves crash fire crackles").split()


def synth_captions(n, seed=7):
    """Synthetic lowercase ASCII captions, 5-15 words."""
    import random
    r = random.Random(seed)
    return [" ".join(r.choice(_WORDS) for _ in range(r.randint(5, 15))) for _ in range(n)]


def synth_caption_tokens(n, context_length=77, seed=7, key="caption_tokens"):
    """Stand-in for tokenised captions when the BPE merge table is not on the box: <SOT>, 6-20 random
    word-piece ids, <EOT>, zero padding (same structure as clip.tokenize output)."""
    g = _gen(seed, key)
    out = torch.zeros(n, context_length, dtype=torch.long)
    lens = torch.randint(6, 21, (n,), generator=g)
    for i in range(n):
        k = int(lens[i])
        out[i, 0] = 49406
        out[i, 1:1 + k] = torch.randint(256, 49406, (k,), generator=g)
        out[i, 1 + k] = 49407
    return out
