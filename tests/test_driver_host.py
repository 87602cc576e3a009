"""Host logic of the file-writing driver (generate_samples_batch.py:125-187): caption table parsing and the
PCM_24 writer, checked with the standard-library wave reader.  CPU only."""
import wave

import numpy as np

from text_to_sound_synthesis_amd.pipeline import Diffsound, write_wav_pcm24


def test_read_tsv_groups_captions(tmp_path):
    p = tmp_path / "val.csv"
    p.write_text("file_name,caption\na.wav,a dog barks\nb.wav,rain falls\na.wav,\"birds, chirping\"\n")
    caps = Diffsound.read_tsv(str(p))
    assert caps == {"a.wav": ["a dog barks", "birds, chirping"], "b.wav": ["rain falls"]}


def test_pcm24_writer_roundtrip(tmp_path):
    x = np.concatenate((np.sin(np.arange(2205) * 0.05) * 0.7, [1.5, -1.5, 0.0, 1.0, -1.0]))
    path = str(tmp_path / "x.wav")
    write_wav_pcm24(path, x, 22050)
    with wave.open(path, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()) == (1, 3, 22050, x.size)
        raw = np.frombuffer(w.readframes(x.size), dtype=np.uint8).reshape(-1, 3).astype(np.int32)
    v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v)
    assert np.abs(v[:2205] / 8388608.0 - x[:2205]).max() <= 0.5 / 8388608.0 + 1e-12
    assert list(v[-5:]) == [8388607, -8388608, 0, 8388607, -8388608]          # clipped, no wrap-around


def test_dalle_sample_control_flow_with_stub_backends():
    """DALLE.sample's host logic (dalle_spec.py:264-343: keys, filter-ratio loop, token slicing, train() at the end) with
    the HIP-backed pieces replaced by recording stubs -- the GPU test compares the real thing with the reference."""
    import pytest
    import torch
    from text_to_sound_synthesis_amd.modeling.dalle import DALLE

    class _Tr(torch.nn.Module):
        num_timesteps = 10
        calls = []

        def sample(self, **kw):
            self.calls.append(kw)
            return {"content_token": kw["content_token"] + int(10 * kw["filter_ratio"]) if kw["content_token"].numel()
                    else torch.zeros(2, 265, dtype=torch.long), "logits": torch.ones(1)}

    m = object.__new__(DALLE)
    torch.nn.Module.__init__(m)
    m.content_info, m.condition_info = {"key": "image"}, {"key": "text"}
    m.transformer = _Tr()
    tokens = torch.arange(2 * 265).view(2, 265)
    m.prepare_condition = lambda batch, condition=None: {"condition_token": None, "condition_embed_token": "E"}
    m.prepare_content = lambda batch, with_mask=False: {"content_token": tokens, "content_quant": torch.zeros(2, 256, 5, 53)}
    m.decode_to_img = lambda tok, zshape, stage="first": ("img", tok.clone(), tuple(zshape))
    batch = {"image": "MEL", "text": ["a", "b"]}
    out = m.sample(batch, filter_ratio=[0, 0.5], content_ratio=[1], return_logits=True, noise_fn="NF", batch_size=2)
    assert sorted(out) == sorted(["condition", "input_image", "reconstruction_image", "cond1_cont1_fr0_image",
                                  "cond1_cont1_fr0.5_image", "logits"])
    assert out["condition"] == ["a", "b"] and out["input_image"] == "MEL" and m.training
    assert torch.equal(out["reconstruction_image"][1], tokens) and out["reconstruction_image"][2] == (2, 256, 5, 53)
    assert torch.equal(out["cond1_cont1_fr0.5_image"][1], tokens + 5)
    c = _Tr.calls
    assert [k["filter_ratio"] for k in c] == [0, 0.5] and all(k["condition_embed"] == "E" and k["noise_fn"] == "NF" for k in c)
    assert all(k["return_logits"] and not k["return_att_weight"] and k["sample_type"] == "normal" for k in c)
    out = m.sample(batch, return_rec=False, filter_ratio=[0], content_ratio=[0.5])        # sliced tokens only from all-mask
    assert "reconstruction_image" not in out and _Tr.calls[-1]["content_token"].shape == (2, 132)
    with pytest.raises(ValueError):
        m.sample(batch, filter_ratio=[0.5], content_ratio=[0.5])
    with pytest.raises(NotImplementedError):
        m.sample(batch, return_att_weight=True)
    with pytest.raises(NotImplementedError):
        m.sample(batch, sample_type="debug")


def test_padded_row_mode_selection_and_workspace():
    """Host logic of the native denoiser handle (csrc/api.hip rows_per_sample / carve; no device work, runs without a GPU):
    the sampling step pads every sample to 272 rows exactly where the per-sample GEMM program serves the batch -- f16x2
    mode, row padding on, and the grid rule of csrc/gemm_f16x2_ps.hip (ds_gemm_f16x2_ps_choice, mirrored below) picks full
    or half tiles for the N = 1024 GEMMs: B = 64 / 128 (full tiles), 32 (half tiles), not 1 / 8 / 16 -- and the workspace
    query covers it."""
    import ctypes as C

    import torch
    from text_to_sound_synthesis_amd import _lib as L
    lib = L.lib()
    d = L.DenoiserDesc()
    d.n_layer, d.n_embd, d.n_head, d.seq_len, d.cond_len, d.cond_dim = 2, 1024, 16, 265, 77, 512
    d.n_codes, d.n_steps, d.mlp_mult = 256, 100, 4
    dummy = torch.zeros(64)                       # host memory: the handle only stores pointers
    for f in ("tok_emb", "pos_emb", "lnf_g", "lnf_b", "w_logits", "b_logits", "sched"):
        setattr(d, f, dummy.data_ptr())
    n = 2 * L.LP_COUNT
    ptrs = (C.c_void_p * n)(*([dummy.data_ptr()] * n))
    h = C.c_void_p()
    L.check(lib.ds_denoiser_create(C.byref(d), ptrs, C.byref(h)))
    try:
        assert [lib.ds_denoiser_rows_per_sample(h, B) for B in (1, 32, 64)] == [265, 265, 265]       # fp32 mode: never
        scales = (C.c_float * n)(*([1.0] * n))
        L.check(lib.ds_denoiser_set_split_weights(h, 2, ptrs, scales, dummy.data_ptr(), 1.0))        # f16x2 mode
        def choice(B, N=1024):                    # share of the occupied CU-rounds that work; x0.92 for half tiles; floor 0.65
            tf, th = B * (N // 256), 2 * B * (N // 256)
            ef, eh = tf / (-(-tf // 256) * 256), 0.92 * th / (-(-th // 256) * 256)
            return 0 if max(ef, eh) < 0.65 else (1 if ef >= eh else 2)
        got = {B: lib.ds_denoiser_rows_per_sample(h, B) for B in range(1, 131)}
        assert got == {B: 272 if choice(B) else 265 for B in range(1, 131)}, got
        assert [got[B] for B in (1, 8, 16, 20, 24, 32, 48, 64, 100, 128)] == [265, 265, 265, 265, 272, 272, 272, 272, 272, 272]
        assert (choice(32), choice(64), choice(48)) == (2, 1, 1)
        ws = {B: lib.ds_denoiser_workspace_bytes(h, B) for B in (8, 64)}
        assert ws[64] >= 64 * 272 * 1024 * 4 * (1 + 1 + 3 + 1 + 4) and ws[64] > 8 * ws[8] * 0.99
        L.check(lib.ds_denoiser_set_row_padding(h, 0))
        assert lib.ds_denoiser_rows_per_sample(h, 64) == 265
        L.check(lib.ds_denoiser_set_row_padding(h, 1))
        assert lib.ds_denoiser_rows_per_sample(h, 64) == 272
        assert lib.ds_denoiser_set_split_weights(h, 1, ptrs, scales, dummy.data_ptr(), 1.0) != 0     # (the removed bf16 split)
        L.check(lib.ds_denoiser_set_split_weights(h, 0, None, None, None, 1.0))                      # back to fp32: never
        assert lib.ds_denoiser_rows_per_sample(h, 64) == 265
    finally:
        lib.ds_denoiser_destroy(h)


# ---- argument rules of the sampling tails and of the denoiser's step / chain entries (csrc/sampler.hip ds_sample_tail_check,
# csrc/api.hip step_check / run_chain).  Parameter names in ABI order; a name's valid value comes from _VALID.
_TAIL_ENTRIES = {
    "ds_sample_tail": "logits xt t u sched out dbg dbg dbg B L K T initial trunc_r stream",
    "ds_sample_tail_ex": "logits xt t u sched out dbg dbg dbg B L K T initial trunc_r trunc_k stream",
    "ds_sample_tail_rng": "logits xt t gids seed call sched out B L K T initial trunc_r trunc_k stream",
    "ds_sample_tail_hold": "logits xt t u sched out dbg dbg dbg B L K T initial trunc_r trunc_k keep known mode stream",
    "ds_sample_tail_hold_rng": "logits xt t gids seed call sched out B L K T initial trunc_r trunc_k keep known mode stream",
    "ds_sample_tail_guided":
        "logits logits_u xt t u sched out dbg dbg dbg B L K T initial trunc_r trunc_k scale keep known mode stream",
    "ds_sample_tail_guided_rng":
        "logits logits_u xt t gids seed call sched out B L K T initial trunc_r trunc_k scale keep known mode stream",
    "ds_sample_tail_purity":
        "logits logits_u? scale xt u remain weight trunc_r trunc_k lrows scratch out dbg dbg dbg B L K stream",
    "ds_sample_tail_purity_rng":
        "logits logits_u? scale xt gids seed call remain weight trunc_r trunc_k lrows scratch out dbg dbg dbg B L K stream",
}
_DENOISER_ENTRIES = {
    "ds_denoiser_step": "h tokens_in t kv u B initial trunc_r workspace tokens_out stream",
    "ds_denoiser_step_ex": "h tokens_in t t_post kv u B initial trunc_r trunc_k workspace tokens_out stream",
    "ds_denoiser_step_rng": "h tokens_in t t_post kv gids seed call B initial trunc_r trunc_k workspace tokens_out stream",
    "ds_denoiser_sample_rng":
        "h tokens tokens_tmp t_steps n_calls kv gids seed call B initial trunc_r trunc_k workspace stream",
    "ds_denoiser_step_hold":
        "h tokens_in t t_post kv u B initial trunc_r trunc_k keep known mode workspace tokens_out stream",
    "ds_denoiser_step_hold_rng":
        "h tokens_in t t_post kv gids seed call B initial trunc_r trunc_k keep known mode workspace tokens_out stream",
    "ds_denoiser_sample_hold_rng":
        "h tokens tokens_tmp t_steps n_calls kv gids seed call B initial trunc_r trunc_k keep known mode workspace stream",
    "ds_denoiser_step_guided":
        "h tokens_in t t_post kv u B initial trunc_r trunc_k scale keep known mode tokens2 workspace tokens_out stream",
    "ds_denoiser_step_guided_rng": "h tokens_in t t_post kv gids seed call B initial trunc_r trunc_k scale keep known mode "
                                   "tokens2 workspace tokens_out stream",
    "ds_denoiser_sample_guided_rng": "h tokens tokens_tmp t_steps n_calls kv gids seed call B initial trunc_r trunc_k scale "
                                     "keep known mode tokens2 workspace stream",
    "ds_denoiser_step_purity":
        "h tokens_in t kv u B remain weight trunc_r trunc_k scale tokens2? workspace scratch tokens_out stream",
    "ds_denoiser_step_purity_rng":
        "h tokens_in t kv gids seed call B remain weight trunc_r trunc_k scale tokens2? workspace scratch tokens_out stream",
    "ds_denoiser_sample_purity_rng": "h tokens tokens_tmp t_steps remains n_calls kv gids seed call B weight trunc_r trunc_k "
                                     "scale tokens2? workspace scratch stream",
}
_PTR = 1 << 20                 # a non-null address that nothing reads: every case below is rejected before any HIP call
_VALID = dict(B=2, L=265, K=256, T=100, initial=0, trunc_r=-1.0, trunc_k=0, seed=7, call=0, mode=0, scale=1.5, remain=10,
              weight=0.5, lrows=265, n_calls=3, stream=None, dbg=None, t_post=None, keep=None, known=None)
_LATE = "the parent rejected it only after the forward was enqueued"
_NEW = "the parent accepted it: a chain of no calls checked less"


def _rejections(name, names):
    """[(overrides, note)]: every argument `name` rejects, from the parameters it has.  note: '' if the parent rejected the
    call before enqueuing too, else what it did."""
    has = lambda n: n in names or n + "?" in names
    denoiser, purity, guided = has("h"), "purity" in name, "guided" in name
    optional = {"dbg", "t_post", "keep", "known", "stream", "logits_u?", "tokens2?"}
    plain = {"B", "L", "K", "T", "initial", "trunc_r", "trunc_k", "seed", "call", "mode", "scale", "remain", "weight",
             "lrows", "n_calls"}
    out = [({n: None}, "") for n in dict.fromkeys(names) if n not in optional and n not in plain]   # required pointers
    late = _LATE if denoiser and not purity else ""          # the parent's drivers left these two to the tail's launcher
    if has("trunc_k"):
        out += [(dict(trunc_r=0.5, trunc_k=3), late), (dict(trunc_k=-1), late)]
    if has("K"):                                             # (a handle's K and L are checked by ds_denoiser_create)
        out += [(dict(K=300), ""), (dict(K=128), "")]
    if has("L") and not purity:
        out += [(dict(L=65536), "")]
    if has("mode"):
        out += [(dict(mode=2), ""), (dict(mode=-1), ""), (dict(keep=_PTR, known=None), "")]
        if has("u"):
            out += [(dict(mode=1), ""), (dict(mode=1, keep=_PTR, known=_PTR), "")]             # renoise on caller uniforms
    guide_on = {"logits_u?": _PTR} if has("lrows") else {"tokens2?": _PTR} if purity else {}
    if has("scale"):
        out += [(dict(guide_on, scale=v), "") for v in (float("nan"), float("inf"), float("-inf"))]
    if guided and not denoiser:
        out += [(dict(B=0), ""), (dict(L=0), ""), (dict(T=0), "")]
    if denoiser:
        out += [(dict(B=0), ""), (dict(B=-1), "")]
    if has("n_calls"):
        out += [(dict(n_calls=-1), "")]
        if not guided:                                       # (the guided chain checked its rules whatever n_calls)
            out += [(dict(n_calls=0, trunc_r=0.5, trunc_k=3), _NEW)]
    if purity:
        bad = [dict(weight=-1.0), dict(weight=float("nan")), dict(weight=float("inf")), dict(B=0)]
        if has("remain"):
            bad += [dict(remain=-1)]
        if has("lrows"):
            bad += [dict(lrows=264), dict(L=289), dict(L=0)]
        if has("remains"):
            bad += [dict(remains=(5, 3, -1))]               # the last call's remain: every call is checked before the first runs
        out += [(b, "") for b in bad]
    return out


def test_sampling_entries_reject_bad_arguments_before_any_hip_call():
    """Every public sampling-tail entry and every denoiser step / chain entry returns -1, names itself in
    ds_last_error_string() and makes no HIP call (there is no device here) for each argument it rejects: a null required
    pointer, u / gids null on the form that needs it, K other than 256 / 512, both truncations, mode outside 0 / 1, renoise on
    caller uniforms, keep without known, a non-finite guidance scale, logits_u null on the guided tails, and for purity
    remain < 0, a negative or non-finite weight, lrows < L, L > 288 and a bad remain[k] at the last index of a chain.  The
    cases the parent of this test's commit treated differently carry a note (_LATE, _NEW); they are asserted like the rest."""
    import ctypes as C

    import torch
    from text_to_sound_synthesis_amd import _lib as L
    lib = L.lib()
    d = L.DenoiserDesc()
    d.n_layer, d.n_embd, d.n_head, d.seq_len, d.cond_len, d.cond_dim = 2, 1024, 16, 265, 77, 512
    d.n_codes, d.n_steps, d.mlp_mult = 256, 100, 4
    dummy = torch.zeros(64)
    for f in ("tok_emb", "pos_emb", "lnf_g", "lnf_b", "w_logits", "b_logits", "sched"):
        setattr(d, f, dummy.data_ptr())
    n = 2 * L.LP_COUNT
    ptrs = (C.c_void_p * n)(*([dummy.data_ptr()] * n))
    h = C.c_void_p()
    L.check(lib.ds_denoiser_create(C.byref(d), ptrs, C.byref(h)))
    entries = dict(_TAIL_ENTRIES, **_DENOISER_ENTRIES)
    assert len(_TAIL_ENTRIES) == 9 and len(_DENOISER_ENTRIES) == 13
    assert sorted(entries) == sorted(k for k in L._PROTOS if k.startswith(("ds_sample_tail", "ds_denoiser_step", "ds_denoiser_sample")))
    problems, total = [], 0
    try:
        for name, spec in entries.items():
            names = spec.split()
            assert len(names) == len(L._PROTOS[name][1]), name
            cases = _rejections(name, names)
            assert len(cases) >= 5, name
            for over, note in cases:
                vals = dict(_VALID, h=h, remains=(5, 3, 0), **{"logits_u?": None, "tokens2?": None})
                vals.update(over)
                if isinstance(vals["remains"], tuple):
                    vals["remains"] = (C.c_int * 3)(*vals["remains"])
                rc = getattr(lib, name)(*[vals.get(p, _PTR) for p in names])
                msg = lib.ds_last_error_string().decode()
                total += 1
                if rc != -1 or name not in msg:
                    problems.append("%s %r -> rc %d, %r%s" % (name, over, rc, msg, " (%s)" % note if note else ""))
    finally:
        lib.ds_denoiser_destroy(h)
    assert not problems, "\n".join(problems)
    assert total > 300


def test_cpu_baseline_reports_what_the_host_gives(tmp_path):
    """the cpu_baseline object names the CPU model, the affinity count and the cgroup CPU quota, and the
    thread sweep stops at what the process may actually use."""
    import os
    import bench
    info = bench.host_cpu_info()
    assert set(info) == {"model", "affinity_cpus", "cgroup_cpu_max", "cgroup_quota_cpus", "numa_nodes_online"}
    assert info["affinity_cpus"] is None or 1 <= info["affinity_cpus"] <= (os.cpu_count() or 1)
    v2 = tmp_path / "v2"
    v2.mkdir()
    (v2 / "cpu.max").write_text("1600000 100000\n")
    assert bench._cgroup_quota(str(v2)) == ("1600000 100000", 16)
    (v2 / "cpu.max").write_text("max 100000\n")
    assert bench._cgroup_quota(str(v2)) == ("max 100000", None)
    v1 = tmp_path / "v1"
    (v1 / "cpu").mkdir(parents=True)
    (v1 / "cpu" / "cpu.cfs_quota_us").write_text("250000\n")
    (v1 / "cpu" / "cpu.cfs_period_us").write_text("100000\n")
    assert bench._cgroup_quota(str(v1)) == ("250000 100000", 3)
    assert bench._cgroup_quota(str(tmp_path / "none")) == (None, None)
