"""End-to-end parity on the MI355X: the drop-in classes (src.*) driven through OneProtLitModule.training_step against
 (a) the golden vectors produced by the reference itself, and (b) the CPU oracle on the same inputs.

Tolerances: bf16-operand MFMA path -> loss rel <= 1e-3, feature cosine >= 0.999,
gradient cosine >= 0.99 on every tensor, post-Adam weights within the lr-sized step."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import oneprot_oracle as O  # noqa: E402
from tests.cases import esm_dir_from_cfg, golden_pair_module  # noqa: E402,F401
from tests.gate import cos_sim  # noqa: E402

DEV = "cuda"


def _build(golden_dir, tag, tmp_path, frozen_seq=False):
    os.environ.update(ONEPROT_ALLOW_RANDOM_INIT="1")
    return golden_pair_module(golden_dir, tag, tmp_path, frozen_seq)


@pytest.mark.parametrize("tag", ["hd16", "hd32", "hd24"])
def test_forward_features_vs_reference(golden_dir, tag, tmp_path):
    g, module = _build(golden_dir, tag, tmp_path)
    with torch.no_grad():
        sf = module(g["seq_ids"].to(DEV), "sequence").cpu()
        mf = module(g["st_ids"].to(DEV), "struct_token").cpu()
    for got, ref, name in ((sf, g["sequence_features"], "sequence"), (mf, g["modality_features"], "struct_token")):
        cs = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
        assert cs.min() > 0.999, f"{name}: min cosine {cs.min()}"
        assert (got - ref).abs().max() < 0.05 * ref.abs().max(), name
    assert abs(mf.norm(dim=-1) - 1 / 0.07).max() < 1e-3


@pytest.mark.parametrize("tag", ["hd16", "hd32", "hd24"])
def test_training_substep_vs_reference(golden_dir, tag, tmp_path):
    g, module = _build(golden_dir, tag, tmp_path)
    batch = {"struct_token": (g["seq_ids"].to(DEV), g["st_ids"].to(DEV), "struct_token", None)}
    # capture gradients before the optimizer consumes them
    grads = {}
    orig_clip = module.clip_gradients

    def spy(opt, **kw):
        for name, enc in module.network.items():
            pref = "seq." if name == "sequence" else "st."
            tr = enc.transformer
            if tr.flat.grad is not None:
                for k in tr._spec:
                    grads[pref + "transformer." + k] = tr.view(k, tr.flat.grad).detach().cpu().clone()
            for k, p_ in enc.proj.named_parameters():
                if p_.grad is not None:
                    grads[pref + "proj." + k] = p_.grad.detach().cpu().clone()
        return orig_clip(opt, **kw)

    module.clip_gradients = spy
    loss = module.training_step(batch, 0)
    loss = float(loss)
    ref_loss = float(g["loss_total"])
    # 1e-3 relative (BASELINE north_star) against the reference's own output, every fixture
    assert abs(loss - ref_loss) / abs(ref_loss) < 1e-3, (loss, ref_loss)
    gn = float(module.last_grad_norm)
    assert abs(gn - float(g["grad_total_norm"])) / float(g["grad_total_norm"]) < 2e-2, (gn, float(g["grad_total_norm"]))
    worst = (1.0, None)
    n = 0
    for k, ref in g["grads"].items():
        if k not in grads:
            assert "pooler" in k or "contact_head" in k, k
            continue
        if ref.abs().max() < 1e-7:
            continue
        c = cos_sim(grads[k], ref)
        worst = min(worst, (c, k))
        n += 1
    assert n > 30
    if os.environ.get("ONEPROT_TEST_VERBOSE"):
        for k, ref in g["grads"].items():
            if k in grads and ref.abs().max() >= 1e-7:
                print(f"{cos_sim(grads[k], ref):.5f} {float(ref.norm()):.3e} {k}")
    # every tensor >= 0.98; tensors carrying a non-negligible share of the gradient (norm >= 1 % of the largest) >= 0.999;
    # the whole gradient as one vector >= 0.9999.  (Tiny q/k gradients are differences of nearly equal bf16-rounded
    # terms, dS = P*(dP - delta), hence the looser per-tensor floor; observed worst 0.989 at |g| = 1e-2 vs 1e+1.)
    assert worst[0] > 0.98, f"worst gradient cosine {worst}"
    big = max(float(v.norm()) for v in g["grads"].values())
    keys = [k for k, ref in g["grads"].items() if k in grads and ref.abs().max() >= 1e-7]
    for k in keys:
        if float(g["grads"][k].norm()) >= 0.01 * big:
            assert cos_sim(grads[k], g["grads"][k]) > 0.999, k
    allg = torch.cat([grads[k].flatten() for k in keys]); allr = torch.cat([g["grads"][k].flatten() for k in keys])
    assert cos_sim(allg, allr) > 0.9999
    # post-Adam weights: step-1 update is lr*sign-ish; compare against the reference's updated tensors
    coef = min(1.0, 1.0 / (float(g["grad_total_norm"]) + 1e-6))
    for enc_name, after, gpref in (("sequence", g["sd_seq_after"], "seq."), ("struct_token", g["sd_st_after"], "st.")):
        sd = {k: v.cpu() for k, v in module.network[enc_name].state_dict().items()}
        for k, v in after.items():
            if "inv_freq" in k or gpref + k not in g["grads"]:
                continue
            # the first Adam step is lr*g/(|g|+eps) ~ lr*sign(g): only elements whose gradient is well above the bf16 noise floor
            # of their tensor (2 % of its max) have a stable sign
            ga = (g["grads"][gpref + k] * coef).abs()
            well = ga > max(1e-4, 0.02 * float(ga.max()))
            if well.any():
                assert (sd[k] - v)[well].abs().max() < 2e-4, k
            assert (sd[k] - v).abs().max() < 2.1e-3, k


def test_seqsim_substep_applies_the_sequence_encoder_twice(golden_dir, tmp_path):
    """`use_seqsim=True` with a TRAINABLE sequence encoder (ref oneprot_module.py:16,84-97): the batch entry "seqsim" sends both inputs through
    network["sequence"], so one encoder is applied twice before one backward -- the multi-application branch of the encoder's autograd node (the
    arena gradient of the second application is accumulated onto the first by autograd; no overlapped reduction).  Checked against the oracle
    applying ONE parameter set twice: loss 1e-3, whole-gradient cosine, gradient norm, the Adam step."""
    g, module = _build(golden_dir, "hd32", tmp_path)
    module.use_seqsim = True
    ids_a = g["seq_ids"]
    gen = torch.Generator().manual_seed(77)
    ids_b = ids_a.clone()
    body = (ids_b >= 4) & (ids_b <= 23)
    ids_b[body] = torch.randint(4, 24, (int(body.sum()),), generator=gen)          # another sequence of the same lengths / padding
    cfg = g["cfg"]
    cfg_o = dict(layers=cfg["layers"], hidden=cfg["hidden"], heads=cfg["heads"], ffn=cfg["ffn"], pad=cfg["pad"], mask=cfg["mask"], eps=cfg["eps"])
    spec = dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False)
    ref = O.train_substep_seqsim(ids_a, ids_b, g["sd_seq"], cfg_o, spec, use_l1=True)
    grads = {}
    orig_clip = module.clip_gradients

    def spy(opt, **kw):
        enc = module.network["sequence"]
        tr = enc.transformer
        for k in tr._spec:
            grads["seq.transformer." + k] = tr.view(k, tr.flat.grad).detach().cpu().clone()
        for k, p_ in enc.proj.named_parameters():
            grads["seq.proj." + k] = p_.grad.detach().cpu().clone()
        assert module.network["struct_token"].transformer.flat.grad is None      # the inactive modality receives nothing
        return orig_clip(opt, **kw)

    module.clip_gradients = spy
    # "struct_token" also in the batch would be a second sub-step; here only the seqsim pair
    loss = float(module.training_step({"seqsim": (ids_a.to(DEV), ids_b.to(DEV), "seqsim", None)}, 0))
    assert abs(loss - float(ref["loss"])) / abs(float(ref["loss"])) < 1e-3, (loss, float(ref["loss"]))
    gn = float(module.last_grad_norm)
    assert abs(gn - float(ref["grad_total_norm"])) / float(ref["grad_total_norm"]) < 2e-2, (gn, float(ref["grad_total_norm"]))
    keys = [k for k, v in ref["grads"].items() if k in grads and v.abs().max() >= 1e-7]
    assert len(keys) > 30
    allg = torch.cat([grads[k].flatten() for k in keys]); allr = torch.cat([ref["grads"][k].flatten() for k in keys])
    assert cos_sim(allg, allr) > 0.9999, cos_sim(allg, allr)
    big = max(float(ref["grads"][k].norm()) for k in keys)
    for k in keys:
        if float(ref["grads"][k].norm()) >= 0.01 * big:
            assert cos_sim(grads[k], ref["grads"][k]) > 0.999, (k, cos_sim(grads[k], ref["grads"][k]))
    sd = {k: v.cpu() for k, v in module.network["sequence"].state_dict().items()}
    for k, v in ref["new_params"].items():
        assert (sd[k[4:]] - v).abs().max() < 2.1e-3, k
    tr = module.network["sequence"].transformer
    assert getattr(tr, "_live_apps", 0) == 0 and not getattr(tr, "_multi_app_step", False)      # bookkeeping of the two applications is back to idle
    # without use_seqsim the entry is skipped, as in the reference (oneprot_module.py:88-90)
    module.use_seqsim = False
    assert module.training_step({"seqsim": (ids_a.to(DEV), ids_b.to(DEV), "seqsim", None)}, 1) is None


def test_frozen_sequence_encoder_gets_no_grad(golden_dir, tmp_path):
    g, module = _build(golden_dir, "hd32", tmp_path, frozen_seq=True)
    before = module.network["sequence"].transformer.flat.detach().clone()
    batch = {"struct_token": (g["seq_ids"].to(DEV), g["st_ids"].to(DEV), "struct_token", None)}
    module.training_step(batch, 0)
    assert module.network["sequence"].transformer.flat.grad is None
    assert torch.equal(before, module.network["sequence"].transformer.flat.detach())
    assert module.network["sequence"].proj[1].weight.grad is not None


def test_full_size_shapes_vs_oracle():
    """ESM-2-8M-shaped encoder (6 layers, d=320, 20 heads, hd=16) at B=4, L=128 (cfg-1 shape, reduced batch): HIP vs CPU oracle."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.struct_token_encoder import StructTokenEncoder
    torch.manual_seed(0)
    enc = StructTokenEncoder("facebook/esm2_t6_8M_UR50D", output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    with torch.no_grad():
        for k, v in enc.transformer.named_views().items():
            if k.endswith(".bias"):
                v.normal_(0, 0.02)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    gen = torch.Generator().manual_seed(1881)
    B, L = 4, 128
    ids = torch.randint(33, 53, (B, L), generator=gen)
    ids[:, 0] = 0
    lens = [128, 100, 37, 128]
    for b, n in enumerate(lens):
        ids[b, n - 1] = 2
        ids[b, n:] = 1
    cfg = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5)
    ref = O.encoder_features("esm", ids, sd, cfg, "mean", "linear", True)
    enc = enc.to(DEV)
    with torch.no_grad():
        got = enc(ids.to(DEV)).cpu()
    cs = torch.nn.functional.cosine_similarity(got, ref, dim=-1)
    assert cs.min() > 0.999, cs


def test_text_encoder_vs_reference(golden_dir, tmp_path):
    """BERT text tower (cls pooling, mlp head, logit scale; frozen, eval) vs the reference's TextEncoder output."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.text_encoder import TextEncoder
    g = torch.load(os.path.join(golden_dir, "bert_text.pt"), weights_only=False)
    cfg = g["cfg"]
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], pooling_type="cls", proj_type="mlp", use_logit_scale=True, learnable_logit_scale=False, frozen=True,
                      use_lora=False)
    enc.transformer.train_dropout = False      # held against the eval-mode reference / oracle (the default follows the reference: HF's train-mode dropout)
    enc.load_state_dict(g["sd"], strict=True)
    enc = enc.to(DEV).eval()
    with torch.no_grad():
        feats = enc(g["ids"].to(DEV)).cpu()
        hidden = enc.transformer(input_ids=g["ids"].to(DEV)).last_hidden_state.cpu()
    mask = (g["ids"] != 0).unsqueeze(-1).float()
    ref_h = g["acts"]["last_hidden"]
    assert ((hidden - ref_h) * mask).abs().max() < 0.05 * ref_h.abs().max()
    cs = torch.nn.functional.cosine_similarity(feats, g["features"], dim=-1)
    assert cs.min() > 0.999, cs
    assert abs(feats.norm(dim=-1) - 1 / 0.07).max() < 1e-3


def _bert_keep_masks(tr, call, B, T):
    """the masks (already divided by the keep probability) the HIP path drew in forward call `call` of a BERT tower running hf's train-mode dropout:
    {"emb": [B, T, d], "layers": [{"attn": [B, H, T, T], "out1": [B, T, d], "out2": [B, T, d]}, ...]} -- the oracle's cfg["bert_keep"]"""
    from oneprot_amd import hip
    d, H, n = tr.d, tr.H, tr.n_layers
    p_h, p_a = float(tr.config.hidden_dropout_prob), float(tr.config.attention_probs_dropout_prob)
    sc = lambda p_: 65536.0 / (65536 - int(p_ * 65536 + 0.5))

    def hidden_keep(layer, site):
        ones = torch.ones(B * T, d, device=DEV)
        out = torch.empty_like(ones)
        hip.call("oneprot_dropout_f32", ones, out, ones.numel(), p_h, tr._drop_seed, tr._drop_stream(call, layer, site))
        return ((out > 0).float() * sc(p_h)).view(B, T, d).cpu()

    layers = []
    for i in range(n):
        kp = torch.empty(B, H, T, T, dtype=torch.uint8, device=DEV)
        hip.call("oneprot_attn_dropout_keep", kp, B, H, T, p_a, tr._drop_seed, tr._drop_stream(call, i, 0))
        layers.append(dict(attn=kp.float().cpu() * sc(p_a), out1=hidden_keep(i, 1), out2=hidden_keep(i, 2)))
    return dict(emb=hidden_keep(-1, 0), layers=layers)


def test_text_encoder_train_mode_dropout_vs_oracle(golden_dir, tmp_path):
    """hf's train-mode dropout of the frozen BERT tower (embeddings, attention probabilities, the two dense outputs per layer; the reference leaves it
    on in train mode: text_encoder.py:59), ON by default in train mode since round 5: last hidden state and features against the oracle handed the masks
    the HIP path drew; `transformer.train_dropout = False` switches it off; eval mode untouched; a second call draws new masks."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from oneprot_amd import hip
    from src.models.components.text_encoder import TextEncoder
    g = torch.load(os.path.join(golden_dir, "bert_text.pt"), weights_only=False)
    cfg = g["cfg"]
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    torch.manual_seed(5)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], pooling_type="cls", proj_type="mlp", use_logit_scale=True, learnable_logit_scale=False, frozen=True,
                      use_lora=False)
    enc.load_state_dict(g["sd"], strict=True)
    enc = enc.to(DEV).train()
    tr = enc.transformer
    ids = g["ids"]
    B, T = ids.shape
    tr.train_dropout = False
    with torch.no_grad():
        plain = enc(ids.to(DEV)).cpu()                                   # switched off: train mode == eval mode
    assert torch.nn.functional.cosine_similarity(plain, g["features"], dim=-1).min() > 0.999
    tr.train_dropout = None                                              # the default: follows the module's train / eval mode, as the reference's tower does
    assert (float(tr.config.hidden_dropout_prob), float(tr.config.attention_probs_dropout_prob)) == (0.1, 0.1)
    with torch.no_grad():
        feats = enc(ids.to(DEV)).cpu()
    keep = _bert_keep_masks(tr, tr._drop_calls - 1, B, T)
    assert abs(float(keep["emb"].gt(0).float().mean()) - 0.9) < 0.02 and abs(float(keep["layers"][0]["attn"].gt(0).float().mean()) - 0.9) < 0.02
    ocfg = dict(cfg, bert_keep=keep)
    rf = O.encoder_features("bert", ids, g["sd"], ocfg, "cls", "mlp", True)
    cs = torch.nn.functional.cosine_similarity(feats, rf, dim=-1)
    assert cs.min() > 0.999, cs
    r0 = O.encoder_features("bert", ids, g["sd"], cfg, "cls", "mlp", True)
    assert torch.nn.functional.cosine_similarity(r0, rf, dim=-1).min() < 0.999          # the masks move the features by more than the parity tolerance
    with torch.no_grad():
        again = enc(ids.to(DEV)).cpu()
        assert not torch.allclose(again, feats, atol=1e-3)                               # new masks on every call
        enc.eval()
        e1 = enc(ids.to(DEV)).cpu()
    assert torch.allclose(e1, plain, atol=1e-6)


def test_trainable_text_encoder_gradients_vs_reference(golden_dir, tmp_path):
    """TextEncoder(frozen=False) (the signature default, ref text_encoder.py:9-37): loss and the gradient of every BERT / head parameter vs the
    reference's autograd, through the hand-written BERT backward (post-LN layers, embedding LayerNorm, sorted embedding-row reduction)."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.text_encoder import TextEncoder
    from src.models.components.loss import ClipLoss
    g = torch.load(os.path.join(golden_dir, "bert_text_train.pt"), weights_only=False)
    cfg = g["cfg"]
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], pooling_type="mean", proj_type="linear", use_logit_scale=True, learnable_logit_scale=False, frozen=False,
                      use_lora=False)
    enc.transformer.train_dropout = False      # held against the eval-mode reference / oracle (the default follows the reference: HF's train-mode dropout)
    enc.load_state_dict(g["sd"], strict=True)
    enc = enc.to(DEV)
    feats = enc(g["ids"].to(DEV))
    cs = torch.nn.functional.cosine_similarity(feats.detach().cpu(), g["features"], dim=-1)
    assert cs.min() > 0.999, cs
    loss = ClipLoss()(g["seq_features"].to(DEV), feats)
    assert abs(float(loss) - float(g["loss"])) / float(g["loss"]) < 2e-3, (float(loss), float(g["loss"]))      # 6 pairs, d=64 (see the hd24 note above)
    loss.backward()
    tr = enc.transformer
    got = {"transformer." + k: tr.view(k, tr.flat.grad).detach().cpu() for k in tr._spec}
    got.update({"proj." + k: p_.grad.detach().cpu() for k, p_ in enc.proj.named_parameters()})
    n = 0
    for k, ref in g["grads"].items():
        assert k in got, k
        if float(ref.norm()) < 1e-6:
            continue
        c = cos_sim(got[k], ref)
        assert c > 0.98, (k, c)
        if float(ref.norm()) > 0.05 * max(float(v.norm()) for v in g["grads"].values()):
            assert c > 0.999, (k, c)
        n += 1
    assert n >= 38
    wg = got["transformer.embeddings.word_embeddings.weight"]
    assert float(wg[cfg["pad"]].abs().max()) == 0.0                      # padding_idx row
    unused = [r for r in range(cfg["vocab"]) if r not in set(g["ids"].flatten().tolist())]
    assert float(wg[unused].abs().max()) == 0.0
    allg = torch.cat([got[k].flatten() for k in g["grads"]]); allr = torch.cat([v.flatten() for v in g["grads"].values()])
    assert cos_sim(allg, allr) > 0.9995


def test_trainable_text_encoder_train_mode_dropout_gradients_vs_oracle(golden_dir, tmp_path):
    """the same option on a TRAINABLE text tower: loss and the gradient of every BERT / head parameter through the four dropouts (hidden masks on the
    dense outputs' gradients, the masked attention backward, the embedding mask) against the oracle's autograd with the exported masks."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.text_encoder import TextEncoder
    from src.models.components.loss import ClipLoss
    g = torch.load(os.path.join(golden_dir, "bert_text_train.pt"), weights_only=False)
    cfg = g["cfg"]
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    torch.manual_seed(6)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], pooling_type="mean", proj_type="linear", use_logit_scale=True, learnable_logit_scale=False, frozen=False,
                      use_lora=False)
    enc.load_state_dict(g["sd"], strict=True)
    enc = enc.to(DEV).train()
    tr = enc.transformer
    tr.train_dropout = True
    tr._rng_uid = 3                                               # (the tower id inside the dropout stream ids: pinned, so that the masks -- and the size of their effect checked below -- do not depend on how many towers this process built before)
    ids = g["ids"]
    feats = enc(ids.to(DEV))
    keep = _bert_keep_masks(tr, tr._drop_calls - 1, *ids.shape)
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in g["sd"].items()}
    rf = O.encoder_features("bert", ids, osd, dict(cfg, bert_keep=keep), "mean", "linear", True)
    rloss = O.clip_loss(g["seq_features"], rf)
    rloss.backward()
    assert torch.nn.functional.cosine_similarity(feats.detach().cpu(), rf.detach(), dim=-1).min() > 0.999
    loss = ClipLoss()(g["seq_features"].to(DEV), feats)
    assert abs(float(loss.detach()) - float(rloss)) / float(rloss) < 2e-3, (float(loss.detach()), float(rloss))
    assert abs(float(rloss) - float(g["loss"])) / float(g["loss"]) > 1e-3          # the masks move the loss by more than the parity tolerance
    loss.backward()
    got = {"transformer." + k: tr.view(k, tr.flat.grad).detach().cpu() for k in tr._spec}
    got.update({"proj." + k: p_.grad.detach().cpu() for k, p_ in enc.proj.named_parameters()})
    refs = {k: v.grad for k, v in osd.items() if v.is_floating_point() and v.grad is not None and k in got}
    big = max(float(v.norm()) for v in refs.values())
    n = 0
    for k, ref in refs.items():
        if float(ref.norm()) < 1e-6:
            continue
        c = cos_sim(got[k], ref)
        assert c > 0.98, (k, c)
        if float(ref.norm()) > 0.05 * big:
            assert c > 0.999, (k, c)
        n += 1
    assert n >= 38
    allg = torch.cat([got[k].flatten() for k in refs]); allr = torch.cat([v.flatten() for v in refs.values()])
    assert cos_sim(allg, allr) > 0.9995


def test_bert_base_shape_trainable_substep_vs_oracle():
    """cfg-4 shape (ESM-2-8M sequence tower <-> BERT-base text tower: 12 layers, d=768, 12 heads of 64, ffn 3072, vocab 30522; cls pooling + mlp head
    as in text.yaml), both towers trainable, 8 ragged pairs (L=64 / T=48): full sub-step loss and gradient norm vs the CPU oracle."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.text_encoder import TextEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(11)
    seq = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    tx = TextEncoder("bert-base-uncased", output_dim=1024, pooling_type="cls", proj_type="mlp", use_logit_scale=True, learnable_logit_scale=False, frozen=False,
                     use_lora=False)
    tx.transformer.train_dropout = False      # held against the eval-mode reference / oracle (the default follows the reference: HF's train-mode dropout)
    with torch.no_grad():
        for k, v in tx.transformer.named_views().items():
            if k.endswith(".bias"):
                v.normal_(0, 0.02)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    sd_tx = {k: v.detach().clone() for k, v in tx.state_dict().items()}
    gen = torch.Generator().manual_seed(1881)
    B, L, T = 8, 64, 48
    seq_ids = torch.randint(4, 24, (B, L), generator=gen)
    seq_ids[:, 0] = 0
    for b, n in enumerate([64, 50, 64, 20, 64, 64, 33, 41]):
        seq_ids[b, n - 1] = 2
        seq_ids[b, n:] = 1
    txt_ids = torch.randint(1000, 30522, (B, T), generator=gen)
    txt_ids[:, 0] = 101
    for b, n in enumerate([48, 30, 48, 7, 48, 19, 48, 40]):
        txt_ids[b, n - 1] = 102
        txt_ids[b, n:] = 0
    txt_ids[1, 3] = txt_ids[5, 9] = txt_ids[0, 2]           # the same word in several rows
    cfg_seq = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5)
    cfg_tx = dict(layers=12, hidden=768, heads=12, ffn=3072, vocab=30522, max_pos=512, pad=0, eps=1e-12)
    ref = O.train_substep(seq_ids, txt_ids, sd_seq, sd_tx, cfg_seq, cfg_tx, dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
                          dict(kind="bert", pooling="cls", proj_type="mlp", use_logit_scale=True), use_l1=True)
    module = OneProtLitModule(components={"sequence": seq, "text": tx}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)
    grads = {}
    orig_clip = module.clip_gradients

    def spy(opt, **kw):
        tr = module.network["text"].transformer
        for k in ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.LayerNorm.weight",
                  "encoder.layer.0.attention.self.query.weight", "encoder.layer.11.output.dense.weight", "encoder.layer.5.attention.output.LayerNorm.bias"):
            grads[k] = tr.view(k, tr.flat.grad).detach().cpu().clone()
        return orig_clip(opt, **kw)

    module.clip_gradients = spy
    loss = float(module.training_step({"text": (seq_ids.to(DEV), txt_ids.to(DEV), "text", None)}, 0).detach())
    assert abs(loss - float(ref["loss"])) / float(ref["loss"]) < 1e-3, (loss, float(ref["loss"]))
    assert abs(float(module.last_grad_norm) - float(ref["grad_total_norm"])) / float(ref["grad_total_norm"]) < 2e-2
    for k, v in grads.items():
        r = ref["grads"]["mod.transformer." + k]
        assert cos_sim(v, r) > 0.98, (k, cos_sim(v, r))


@pytest.mark.parametrize("frozen_seq", [True, False])
def test_multi_step_training_tracks_oracle(golden_dir, tmp_path, frozen_seq):
    """4 consecutive sub-steps (optimizer state, bf16 weight-mirror refresh after each step, frozen / trainable sequence encoder):
    per-step loss within 1e-3 relative of the CPU oracle running torch.optim.Adam on the same start point."""
    g, module = _build(golden_dir, "hd32", tmp_path, frozen_seq=frozen_seq)
    cfg = g["cfg"]
    ref_losses, _, ref_mod = O.train_multi_substeps(g["seq_ids"], g["st_ids"], g["sd_seq"], g["sd_st"], cfg, cfg,
                                                    dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
                                                    dict(kind="esm", pooling="mean", proj_type="linear", use_logit_scale=True), n_steps=4, frozen_seq=frozen_seq)
    batch = {"struct_token": (g["seq_ids"].to(DEV), g["st_ids"].to(DEV), "struct_token", None)}
    got = [float(module.training_step(batch, i).detach()) for i in range(4)]
    # step 1 is a pure function of the inputs: 1e-3.  From step 2 on the trajectories separate slowly: the first Adam updates are
    # ~lr*sign(g), so elements whose gradient is below the bf16 noise floor move by +-lr in either run (observed 1.4e-3 .. 8e-3).
    assert abs(got[0] - ref_losses[0]) / ref_losses[0] < 1e-3, (got, ref_losses)
    for a, b in zip(got[1:], ref_losses[1:]):
        assert abs(a - b) / abs(b) < 2e-2, (got, ref_losses)
    assert got[-1] < got[0]                   # it learns
    assert module.global_step == 4
    # self-consistency AFTER the optimizer steps (catches a stale bf16 weight mirror / transposed copies): the HIP forward on the
    # module's current weights vs the oracle evaluated on those same weights
    sd_seq = {k: v.detach().cpu() for k, v in module.network["sequence"].state_dict().items()}
    sd_st = {k: v.detach().cpu() for k, v in module.network["struct_token"].state_dict().items()}
    with torch.no_grad():
        sf = module(g["seq_ids"].to(DEV), "sequence").cpu()
        mf = module(g["st_ids"].to(DEV), "struct_token").cpu()
    rs = O.encoder_features("esm", g["seq_ids"], sd_seq, cfg, "mean", "mlp", False)
    rm = O.encoder_features("esm", g["st_ids"], sd_st, cfg, "mean", "linear", True)
    assert torch.nn.functional.cosine_similarity(sf, rs, dim=-1).min() > 0.999
    assert torch.nn.functional.cosine_similarity(mf, rm, dim=-1).min() > 0.999
    l_hip, l_ref = float(O.clip_loss(sf, mf)), float(O.clip_loss(rs, rm))
    assert abs(l_hip - l_ref) / l_ref < 1e-3
    moved = (sd_st["transformer.encoder.layer.1.output.dense.weight"] - g["sd_st"]["transformer.encoder.layer.1.output.dense.weight"]).abs().max()
    assert 1e-3 < moved < 4.5e-3              # 4 Adam steps of lr 1e-3


def test_cfg1_shape_train_step_vs_oracle():
    """BASELINE cfg-1 at its own size (ESM-2-8M x2, L=128, batch 32, ragged padding): full sub-step loss + gradient norm vs the CPU oracle."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(3)
    name = "facebook/esm2_t6_8M_UR50D"
    seq = SequenceEncoder(name, output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    st = StructTokenEncoder(name, output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    sd_st = {k: v.detach().clone() for k, v in st.state_dict().items()}
    gen = torch.Generator().manual_seed(1881)
    B, L = 32, 128
    seq_ids = torch.randint(4, 24, (B, L), generator=gen); st_ids = torch.randint(33, 53, (B, L), generator=gen)
    lens = [128, 90, 128, 31, 128, 128, 64, 100] + [int(n) for n in torch.randint(L // 4, L + 1, (B - 8,), generator=gen)]
    for ids in (seq_ids, st_ids):
        ids[:, 0] = 0
        for b, n in enumerate(lens):
            ids[b, n - 1] = 2
            ids[b, n:] = 1
    cfg = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5)
    ref = O.train_substep(seq_ids, st_ids, sd_seq, sd_st, cfg, cfg, dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
                          dict(kind="esm", pooling="mean", proj_type="linear", use_logit_scale=True), use_l1=True)
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)
    loss = float(module.training_step({"struct_token": (seq_ids.to(DEV), st_ids.to(DEV), "struct_token", None)}, 0).detach())
    assert abs(loss - float(ref["loss"])) / float(ref["loss"]) < 1e-3
    assert abs(float(module.last_grad_norm) - float(ref["grad_total_norm"])) / float(ref["grad_total_norm"]) < 2e-2


def test_esm2_35m_shape_train_step_vs_oracle():
    """ESM-2-35M shape (12 layers, d=480, 20 heads, head_dim 24 -- the StructTokenEncoder default model, ref struct_token_encoder.py:9;
    runs on the hd=32 kernels through the padded-head operand layout of oneprot_amd/esm.py), L=128, 8 ragged pairs: full sub-step
    loss, gradient norm and per-tensor gradients of the attention parameters vs the CPU oracle."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(5)
    name = "facebook/esm2_t12_35M_UR50D"
    seq = SequenceEncoder(name, output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    st = StructTokenEncoder(name, output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    assert st.transformer.hd == 24 and st.transformer.hdp == 32
    with torch.no_grad():
        for enc in (seq, st):
            for k, v in enc.transformer.named_views().items():
                if k.endswith(".bias"):
                    v.normal_(0, 0.02)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    sd_st = {k: v.detach().clone() for k, v in st.state_dict().items()}
    gen = torch.Generator().manual_seed(1881)
    B, L = 8, 128
    seq_ids = torch.randint(4, 24, (B, L), generator=gen); st_ids = torch.randint(33, 53, (B, L), generator=gen)
    for ids in (seq_ids, st_ids):
        ids[:, 0] = 0
        for b, n in enumerate([128, 90, 128, 31, 128, 128, 64, 100]):
            ids[b, n - 1] = 2
            ids[b, n:] = 1
    cfg = dict(layers=12, hidden=480, heads=20, ffn=1920, pad=1, mask=32, eps=1e-5)
    ref = O.train_substep(seq_ids, st_ids, sd_seq, sd_st, cfg, cfg, dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
                          dict(kind="esm", pooling="mean", proj_type="linear", use_logit_scale=True), use_l1=True)
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True, local_loss=True, gather_with_grad=True).to(DEV)
    grads = {}
    orig_clip = module.clip_gradients

    def spy(opt, **kw):
        tr = module.network["struct_token"].transformer
        for k in tr._spec:
            if "attention" in k and ("layer.0." in k or "layer.11." in k):
                grads[k] = tr.view(k, tr.flat.grad).detach().cpu().clone()
        return orig_clip(opt, **kw)

    module.clip_gradients = spy
    loss = float(module.training_step({"struct_token": (seq_ids.to(DEV), st_ids.to(DEV), "struct_token", None)}, 0).detach())
    assert abs(loss - float(ref["loss"])) / float(ref["loss"]) < 1e-3, (loss, float(ref["loss"]))
    assert abs(float(module.last_grad_norm) - float(ref["grad_total_norm"])) / float(ref["grad_total_norm"]) < 2e-2
    assert len(grads) == 20
    for k, v in grads.items():
        r = ref["grads"]["mod.transformer." + k]
        if float(r.norm()) > 1e-6:
            assert cos_sim(v, r) > 0.98, (k, cos_sim(v, r))


def test_lora_sequence_encoder_vs_oracle():
    """SequenceEncoder with its signature defaults (use_lora=True, r=8, alpha=16, targets q/k/v, frozen base; ref sequence_encoder.py:23-74): peft's
    key layout, features, adapter / bias gradients (peft bias="all") vs the oracle's restatement of peft 0.5.0 lora.Linear (parity unpinned: peft is
    absent here), and an optimizer step that leaves every non-bias base weight bit-identical."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(21)
    enc = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=256, pooling_type="mean", proj_type="mlp", lora_dropout=0.0)       # use_lora=True, frozen=True by default; the dropout branch has its own test below
    tr = enc.transformer
    with torch.no_grad():
        tr.lora_B.normal_(0, 0.05)                       # peft initialises B = 0 (adapter inactive); make it count
        for k, v in tr.named_views().items():
            if k.endswith(".bias"):
                v.normal_(0, 0.02)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    assert sd["transformer.base_model.model.encoder.layer.0.attention.self.query.lora_A.default.weight"].shape == (8, 320)
    assert sd["transformer.base_model.model.encoder.layer.5.attention.self.value.lora_B.default.weight"].shape == (320, 8)
    assert "transformer.base_model.model.encoder.layer.0.attention.self.query.weight" in sd and "transformer.flat" not in sd
    trainable = sorted(n for n, p_ in enc.named_parameters() if p_.requires_grad)
    assert trainable == sorted(["transformer.flat", "transformer.lora_A", "transformer.lora_B"] + ["proj." + n for n, _ in enc.proj.named_parameters()])
    # a second instance loads the PeftModel-style state dict strictly
    enc2 = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=256, pooling_type="mean", proj_type="mlp", lora_dropout=0.0)
    enc2.load_state_dict(sd, strict=True)
    assert torch.equal(enc2.transformer.lora_B, tr.lora_B.cpu()) and torch.equal(enc2.transformer.flat, tr.flat.cpu())

    gen = torch.Generator().manual_seed(1881)
    B, L = 6, 96
    ids = torch.randint(4, 24, (B, L), generator=gen)
    ids[:, 0] = 0
    for b, n in enumerate([96, 40, 96, 17, 70, 96]):
        ids[b, n - 1] = 2
        ids[b, n:] = 1
    other = torch.nn.functional.normalize(torch.randn(B, 256, generator=gen), dim=-1) * (1 / 0.07)
    cfg = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5, lora_scaling=16 / 8)
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and ("lora_" in k or "bias" in k or k.startswith("proj.")) else v) for k, v in sd.items()}
    rf = O.encoder_features("esm", ids, osd, cfg, "mean", "mlp", False)
    rloss = O.clip_loss(rf, other)
    rloss.backward()

    enc = enc.to(DEV)
    feats = enc(ids.to(DEV))
    cs = torch.nn.functional.cosine_similarity(feats.detach().cpu(), rf.detach(), dim=-1)
    assert cs.min() > 0.999, cs
    from src.models.components.loss import ClipLoss
    loss = ClipLoss()(feats, other.to(DEV))
    assert abs(float(loss) - float(rloss)) / float(rloss) < 2e-3, (float(loss), float(rloss))
    opt = FusedAdam([p_ for p_ in enc.parameters() if p_.requires_grad], lr=1e-3)
    before = tr.flat.detach().clone()
    loss.backward()
    P = "transformer.base_model.model.encoder.layer."
    for i in (0, 5):
        for ti, t in enumerate(("query", "key", "value")):
            for which, got in (("A", tr.lora_A.grad[i, ti]), ("B", tr.lora_B.grad[i, ti])):
                ref = osd[f"{P}{i}.attention.self.{t}.lora_{which}.default.weight"].grad
                assert cos_sim(got.cpu(), ref) > 0.98, (i, t, which, cos_sim(got.cpu(), ref))
    gflat = tr.flat.grad
    idx = tr._lora_bias_index
    mask = torch.zeros_like(gflat, dtype=torch.bool); mask[idx] = True
    assert float(gflat[~mask].abs().max()) == 0.0                                   # frozen base weights, LayerNorm gains: no gradient
    for name in ("encoder.layer.0.attention.self.query.bias", "encoder.layer.3.intermediate.dense.bias", "encoder.layer.5.LayerNorm.bias", "encoder.emb_layer_norm_after.bias"):
        ref = osd["transformer.base_model.model." + name].grad
        assert cos_sim(tr.view(name, gflat).cpu(), ref) > 0.98, name
    opt.step()
    after = tr.flat.detach()
    assert torch.equal(after[~mask], before[~mask]) and not torch.equal(after[mask], before[mask])
    # the merged bf16 operands follow the adapters: features change after the step and still track the oracle evaluated on the new weights
    with torch.no_grad():
        f2 = enc(ids.to(DEV)).cpu()
    sd2 = {k: v.detach().cpu() for k, v in enc.state_dict().items()}
    r2 = O.encoder_features("esm", ids, sd2, cfg, "mean", "mlp", False)
    assert torch.nn.functional.cosine_similarity(f2, r2, dim=-1).min() > 0.999
    assert not torch.allclose(f2, feats.detach().cpu(), atol=1e-4)


def _lora_keep_masks(tr, call_id, B, L):
    """{layer: {target: keep multiplier [B, L, d]}} of forward call `call_id` of a LoRA transformer in train mode: the mask the HIP path drew for
    every adapter's dropout module (regenerated from (seed, call, layer, target) by running the dropout kernel on ones), times 1 / keep probability."""
    from oneprot_amd import hip
    d, p_ = tr.d, float(tr._lora["dropout"])
    thr = int(p_ * 65536 + 0.5)
    ones = torch.ones(B * L, d, dtype=torch.bfloat16, device=DEV)
    out = torch.empty_like(ones)
    keep = {}
    for i in range(tr.n_layers):
        keep[i] = {}
        for ti, t in enumerate(tr._lora["targets"]):
            hip.call("oneprot_dropout_bf16", ones, out, ones.numel(), p_, tr._lora_seed, tr._lora_stream(call_id, i, ti))
            keep[i][t] = ((out.float() > 0).float() * (65536.0 / (65536 - thr))).view(B, L, d).cpu()
    return keep


def test_lora_dropout_two_branch_sequence_encoder_vs_oracle():
    """Train mode with lora_dropout > 0 (the reference's configuration when use_lora is on: sequence.yaml:10, ref sequence_encoder.py:61-74): peft keeps
    the adapter branch apart and feeds it dropout(x), one dropout module per wrapped Linear.  The HIP path's masks are exported and handed to the
    oracle's restatement of peft's forward: features, loss and adapter / bias gradients must agree; eval mode is the merged (mask-free) form."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.loss import ClipLoss
    torch.manual_seed(22)
    enc = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=256, pooling_type="mean", proj_type="mlp", lora_r=4, lora_alpha=8, lora_dropout=0.25)
    tr = enc.transformer
    with torch.no_grad():
        tr.lora_B.normal_(0, 0.08)
        tr.lora_A.mul_(3.0)                               # a branch large enough for its masks to matter
        for k, v in tr.named_views().items():
            if k.endswith(".bias"):
                v.normal_(0, 0.02)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    gen = torch.Generator().manual_seed(1882)
    B, L = 6, 96
    ids = torch.randint(4, 24, (B, L), generator=gen)
    ids[:, 0] = 0
    for b, n in enumerate([96, 40, 96, 17, 70, 96]):
        ids[b, n - 1] = 2
        ids[b, n:] = 1
    other = torch.nn.functional.normalize(torch.randn(B, 256, generator=gen), dim=-1) * (1 / 0.07)
    enc = enc.to(DEV).train()
    call = tr._lora_calls
    feats = enc(ids.to(DEV))
    assert tr._lora_calls == call + 1
    keep = _lora_keep_masks(tr, call, B, L)
    frac = torch.stack([m.gt(0).float().mean() for lay in keep.values() for m in lay.values()])
    assert (frac - 0.75).abs().max() < 0.01, frac                         # keep probability 1 - p
    assert not torch.equal(keep[0]["query"], keep[0]["key"]) and not torch.equal(keep[0]["query"], keep[1]["query"])      # one mask per wrapped Linear
    cfg = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5, lora_scaling=8 / 4, lora_keep=keep)
    osd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and ("lora_" in k or "bias" in k or k.startswith("proj.")) else v) for k, v in sd.items()}
    rf = O.encoder_features("esm", ids, osd, cfg, "mean", "mlp", False)
    rloss = O.clip_loss(rf, other)
    rloss.backward()
    cs = torch.nn.functional.cosine_similarity(feats.detach().cpu(), rf.detach(), dim=-1)
    assert cs.min() > 0.999, cs
    # the masks matter: the mask-free forward of the same weights is measurably elsewhere
    r0 = O.encoder_features("esm", ids, {k: v.detach() for k, v in osd.items()}, dict(cfg, lora_keep=None), "mean", "mlp", False)
    assert torch.nn.functional.cosine_similarity(r0, rf.detach(), dim=-1).min() < 0.9995
    loss = ClipLoss()(feats, other.to(DEV))
    assert abs(float(loss) - float(rloss)) / float(rloss) < 2e-3, (float(loss), float(rloss))
    loss.backward()
    P = "transformer.base_model.model.encoder.layer."
    for i in (0, 3, 5):
        for ti, t in enumerate(("query", "key", "value")):
            for which, got in (("A", tr.lora_A.grad[i, ti]), ("B", tr.lora_B.grad[i, ti])):
                ref = osd[f"{P}{i}.attention.self.{t}.lora_{which}.default.weight"].grad
                assert cos_sim(got.cpu(), ref) > 0.98, (i, t, which, cos_sim(got.cpu(), ref))
    gflat = tr.flat.grad
    idx = tr._lora_bias_index
    mask = torch.zeros_like(gflat, dtype=torch.bool); mask[idx] = True
    assert float(gflat[~mask].abs().max()) == 0.0
    for name in ("encoder.layer.0.attention.self.query.bias", "encoder.layer.3.intermediate.dense.bias", "encoder.layer.5.LayerNorm.bias"):
        ref = osd["transformer.base_model.model." + name].grad
        assert cos_sim(tr.view(name, gflat).cpu(), ref) > 0.98, name
    # a second train-mode call draws new masks; eval mode is deterministic and equals the oracle without masks
    with torch.no_grad():
        f2 = enc(ids.to(DEV)).cpu()
        assert not torch.allclose(f2, feats.detach().cpu(), atol=1e-3)
        enc.eval()
        e1, e2 = enc(ids.to(DEV)).cpu(), enc(ids.to(DEV)).cpu()
    assert torch.equal(e1, e2)
    assert torch.nn.functional.cosine_similarity(e1, r0, dim=-1).min() > 0.999


@pytest.mark.parametrize("lora_dropout", [0.0, 0.2], ids=["merged", "two_branch_dropout"])
def test_lora_text_encoder_vs_oracle(golden_dir, tmp_path, lora_dropout):
    """TextEncoder(use_lora=True, frozen=True) (ref text_encoder.py:39-52): BERT tower with q/k/v adapters -- features and adapter gradients vs the oracle;
    with lora_dropout > 0 in train mode through peft's two-branch form, the oracle fed the masks the HIP path drew."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.text_encoder import TextEncoder
    from src.models.components.loss import ClipLoss
    g = torch.load(os.path.join(golden_dir, "bert_text_train.pt"), weights_only=False)
    cfg = dict(g["cfg"], lora_scaling=16 / 4)
    path = os.path.join(str(tmp_path), "bert")
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=cfg["vocab"], hidden_size=cfg["hidden"], num_hidden_layers=cfg["layers"], num_attention_heads=cfg["heads"],
                       intermediate_size=cfg["ffn"], max_position_embeddings=cfg["max_pos"], pad_token_id=cfg["pad"], layer_norm_eps=cfg["eps"]), f)
    enc = TextEncoder(path, output_dim=cfg["output_dim"], pooling_type="mean", proj_type="linear", use_logit_scale=True, frozen=True, use_lora=True, lora_r=4,
                      lora_alpha=16, lora_dropout=lora_dropout)
    enc.transformer.train_dropout = False      # held against the eval-mode reference / oracle (the default follows the reference: HF's train-mode dropout)
    enc.load_state_dict(g["sd"], strict=False)           # base weights from the (adapter-free) fixture; adapters stay at their init
    with torch.no_grad():
        enc.transformer.lora_B.normal_(0, 0.05)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    osd = {k: (v.clone().requires_grad_(True) if "lora_" in k else v) for k, v in sd.items()}
    enc = enc.to(DEV).train()
    call = enc.transformer._lora_calls
    feats = enc(g["ids"].to(DEV))
    if lora_dropout > 0:
        cfg = dict(cfg, lora_keep=_lora_keep_masks(enc.transformer, call, *g["ids"].shape))
    rf = O.encoder_features("bert", g["ids"], osd, cfg, "mean", "linear", True)
    rloss = O.clip_loss(g["seq_features"], rf)
    rloss.backward()
    assert torch.nn.functional.cosine_similarity(feats.detach().cpu(), rf.detach(), dim=-1).min() > 0.999
    ClipLoss()(g["seq_features"].to(DEV), feats).backward()
    tr = enc.transformer
    for i in range(cfg["layers"]):
        for ti, t in enumerate(("query", "key", "value")):
            for which, got in (("A", tr.lora_A.grad[i, ti]), ("B", tr.lora_B.grad[i, ti])):
                ref = osd[f"transformer.base_model.model.encoder.layer.{i}.attention.self.{t}.lora_{which}.default.weight"].grad
                assert cos_sim(got.cpu(), ref) > 0.98, (i, t, which)


def test_max_length_sequences_vs_oracle():
    """L = 1026 (ESM-2's max_position_embeddings; five attention key chunks, the last one partial), ragged to 700 / 257 tokens: sub-step loss and
    gradient norm vs the CPU oracle."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(3)
    name = "facebook/esm2_t6_8M_UR50D"
    seq = SequenceEncoder(name, output_dim=1024, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=False)
    st = StructTokenEncoder(name, output_dim=1024, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    sd_seq = {k: v.detach().clone() for k, v in seq.state_dict().items()}
    sd_st = {k: v.detach().clone() for k, v in st.state_dict().items()}
    gen = torch.Generator().manual_seed(1881)
    B, L = 3, 1026
    seq_ids = torch.randint(4, 24, (B, L), generator=gen); st_ids = torch.randint(33, 53, (B, L), generator=gen)
    for ids in (seq_ids, st_ids):
        ids[:, 0] = 0
        for b, n in enumerate([1026, 700, 257]):
            ids[b, n - 1] = 2
            ids[b, n:] = 1
    cfg = dict(layers=6, hidden=320, heads=20, ffn=1280, pad=1, mask=32, eps=1e-5)
    ref = O.train_substep(seq_ids, st_ids, sd_seq, sd_st, cfg, cfg, dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
                          dict(kind="esm", pooling="mean", proj_type="linear", use_logit_scale=True), use_l1=True)
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True).to(DEV)
    loss = float(module.training_step({"struct_token": (seq_ids.to(DEV), st_ids.to(DEV), "struct_token", None)}, 0).detach())
    assert abs(loss - float(ref["loss"])) / float(ref["loss"]) < 1e-3, (loss, float(ref["loss"]))
    assert abs(float(module.last_grad_norm) - float(ref["grad_total_norm"])) / float(ref["grad_total_norm"]) < 2e-2


def test_mixed_batch_round_robin(golden_dir, tmp_path):
    """CombinedLoader('min_size') batches with two modalities (struct_token, text): one optimiser sub-step per modality per batch
    (ref oneprot_module.py:84-92), frozen text tower untouched, warm-up gate `train_on_all_modalities_after_step`."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from oneprot_amd.data import CombinedLoader, SyntheticPairs
    from oneprot_amd.optim import FusedAdam
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.components.struct_token_encoder import StructTokenEncoder
    from src.models.components.text_encoder import TextEncoder
    from src.models.oneprot_module import OneProtLitModule
    g = torch.load(os.path.join(golden_dir, "esm_pair_hd16.pt"), weights_only=False)
    tb = torch.load(os.path.join(golden_dir, "bert_text.pt"), weights_only=False)
    p = esm_dir_from_cfg(str(tmp_path), g["cfg"], "esm")
    pb = os.path.join(str(tmp_path), "bert"); os.makedirs(pb)
    c = tb["cfg"]
    with open(os.path.join(pb, "config.json"), "w") as f:
        json.dump(dict(model_type="bert", vocab_size=c["vocab"], hidden_size=c["hidden"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                       intermediate_size=c["ffn"], max_position_embeddings=c["max_pos"], pad_token_id=0, layer_norm_eps=c["eps"]), f)
    seq = SequenceEncoder(p, output_dim=48, pooling_type="mean", proj_type="mlp", use_lora=False, frozen=True)
    st = StructTokenEncoder(p, output_dim=48, pooling_type="mean", proj_type="linear", use_logit_scale=True)
    tx = TextEncoder(pb, output_dim=48, pooling_type="cls", proj_type="mlp", use_logit_scale=True, frozen=True, use_lora=False)
    tx.transformer.train_dropout = False      # held against the eval-mode reference / oracle (the default follows the reference: HF's train-mode dropout)
    seq.load_state_dict(g["sd_seq"]); st.load_state_dict(g["sd_st"]); tx.load_state_dict(tb["sd"])
    module = OneProtLitModule(components={"sequence": seq, "struct_token": st, "text": tx}, optimizer=functools.partial(FusedAdam, lr=1e-3), loss_fn="CLIP",
                              use_l1_regularization=True, train_on_all_modalities_after_step=1).to(DEV)
    loader = CombinedLoader({"struct_token": SyntheticPairs("struct_token", 6, 24, n_batches=3, device=DEV, ragged=True),
                             "text": SyntheticPairs("text", 6, 24, mod_len=20, n_batches=3, device=DEV, ragged=True, text_vocab=c["vocab"])}, "min_size")
    text_before = module.network["text"].transformer.flat.detach().clone()
    text_head_before = module.network["text"].proj[1].weight.detach().clone()
    st_before = module.network["struct_token"].transformer.flat.detach().clone()
    sds0 = {k: {n: v.detach().cpu().clone() for n, v in module.network[k].state_dict().items()} for k in ("sequence", "struct_token", "text")}
    per_substep = []

    class _Recorder(type(module.train_loss)):           # the module's running-mean metric, additionally keeping every sub-step's value
        def __call__(self, value):
            per_substep.append(value.detach().clone())
            super().__call__(value)

    module.train_loss = _Recorder()
    loss = module.fit_steps(loader)
    # batch 0: warm-up gate -> struct_token only (1 sub-step); batches 1, 2: both modalities (2 sub-steps each)
    assert module.global_step == 5
    assert torch.isfinite(loss)
    assert torch.equal(text_before, module.network["text"].transformer.flat.detach())            # frozen tower
    assert not torch.equal(text_head_before, module.network["text"].proj[1].weight.detach())      # its projection head trains
    assert not torch.equal(st_before, module.network["struct_token"].transformer.flat.detach())
    # ---- value level: every sub-step's loss vs the oracle's round-robin loop (one Adam over all components, per-modality sub-steps, warm-up gate)
    cfg_b = dict(layers=c["layers"], hidden=c["hidden"], heads=c["heads"], ffn=c["ffn"], vocab=c["vocab"], max_pos=c["max_pos"], pad=0, eps=c["eps"])
    cfgs = {"sequence": g["cfg"], "struct_token": g["cfg"], "text": cfg_b}
    specs = {"sequence": dict(kind="esm", pooling="mean", proj_type="mlp", use_logit_scale=False),
             "struct_token": dict(kind="esm", pooling="mean", proj_type="linear", use_logit_scale=True),
             "text": dict(kind="bert", pooling="cls", proj_type="mlp", use_logit_scale=True)}
    batches = [{m: (b[0].cpu(), b[1].cpu()) for m, b in batch.items()} for batch in loader]
    ref_log, ref_params = O.train_round_robin(batches, sds0, cfgs, specs, use_l1=True, frozen=("sequence", "text"), train_on_all_modalities_after_step=1)
    assert [m for m, _ in ref_log] == ["struct_token", "struct_token", "text", "struct_token", "text"]
    got = [float(v) for v in per_substep]
    assert len(got) == len(ref_log) == 5
    # sub-steps 0 and 2 are the first time their modality's loss is evaluated (pure functions of the start point up to the shared sequence
    # head): 1e-3; later ones follow Adam updates that are ~lr*sign(g), where bf16-noise sign flips on tiny gradients separate the two
    # trajectories slowly (same gate as test_multi_step_training_tracks_oracle)
    for i, ((m, r), v) in enumerate(zip(ref_log, got)):
        assert abs(v - r) / r < (1e-3 if i == 0 else 2e-2), (i, m, v, r)
    # ---- validation / test hooks: VALUES vs the oracle evaluated on the module's current weights (ref oneprot_module.py:110-121, 137-146)
    sd_now = {k: {n: v.detach().cpu() for n, v in module.network[k].state_dict().items()} for k in ("sequence", "text", "struct_token")}
    vb = next(iter(SyntheticPairs("text", 6, 24, mod_len=20, device=DEV, text_vocab=c["vocab"], seed=77, ragged=True)))
    v_ref, sf_ref, mf_ref = O.validation_substep(vb[0].cpu(), vb[1].cpu(), sd_now["sequence"], sd_now["text"], cfgs["sequence"], cfgs["text"], specs["sequence"], specs["text"])
    v_got = module.validation_step(vb, 0)
    assert abs(float(v_got) - float(v_ref)) / float(v_ref) < 1e-3, (float(v_got), float(v_ref))
    assert abs(float(module.val_loss.compute()) - float(v_ref)) / float(v_ref) < 1e-3
    met = module.metrics["val_text"].compute()
    ref_met = O.retrieval_metrics(sf_ref, mf_ref)
    assert set(met) == set(ref_met)
    t_ref, _, _ = O.test_substep(vb[0].cpu(), vb[1].cpu(), sd_now["sequence"], sd_now["text"], cfgs["sequence"], cfgs["text"], specs["sequence"], specs["text"])
    out = module.test_step({"text": vb}, 0)
    # the reference's double logit scale (14.29^2 on the logits) makes this loss ~20x more sensitive to feature rounding than the training loss
    assert float(t_ref) > 2 * float(v_ref)
    assert abs(float(out["text"]) - float(t_ref)) / float(t_ref) < 2e-2, (float(out["text"]), float(t_ref))
    sb = next(iter(SyntheticPairs("struct_token", 6, 24, device=DEV, seed=78, ragged=True)))
    t2_ref, _, _ = O.test_substep(sb[0].cpu(), sb[1].cpu(), sd_now["sequence"], sd_now["struct_token"], cfgs["sequence"], cfgs["struct_token"], specs["sequence"], specs["struct_token"])
    out2 = module.test_step({"struct_token": sb}, 1)
    assert abs(float(out2["struct_token"]) - float(t2_ref)) / float(t2_ref) < 2e-2
    module.on_validation_epoch_end(); module.on_test_epoch_end()
    assert "val/seq_to_mod_R@1/val_text" in module.logged and "test/mod_to_seq_median_rank/test_struct_token" in module.logged


@pytest.mark.parametrize("frozen", [True, False])
def test_attention1d_pooling_and_learnable_logit_scale(tmp_path, frozen):
    """ref configs/experiment/train_ddp_1.yaml:46 shape in miniature: sequence encoder with pooling_type=attention1d (conv width hard-coded
    1280 in the reference, so the encoder width must be 1280), linear head, learnable logit scale; gradients vs the oracle's autograd."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    cfg = dict(vocab=33, hidden=1280, layers=1, heads=20, ffn=256, pad=1, mask=32, eps=1e-5)
    p = esm_dir_from_cfg(str(tmp_path), cfg, "esm1280")
    torch.manual_seed(5)
    enc = SequenceEncoder(p, output_dim=64, pooling_type="attention1d", proj_type="linear", use_logit_scale=True, learnable_logit_scale=True, use_lora=False,
                          frozen=frozen)
    with torch.no_grad():
        enc.pooling.layer.weight.normal_(0, 0.05)
        enc.pooling.layer.bias.fill_(0.3)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    assert "pooling.layer.weight" in sd and tuple(sd["pooling.layer.weight"].shape) == (1, 1280, 1) and "norm.1.log_logit_scale" in sd
    gen = torch.Generator().manual_seed(2)
    B, L = 3, 24
    ids = torch.randint(4, 24, (B, L), generator=gen)
    ids[:, 0] = 0
    for b, n in enumerate([24, 11, 5]):
        ids[b, n - 1] = 2
        ids[b, n:] = 1
    tgt = torch.randn(B, 64, generator=gen)
    # oracle
    leaf = {k: v.clone().requires_grad_(v.is_floating_point() and "inv_freq" not in k) for k, v in sd.items()}
    ref = O.encoder_features("esm", ids, leaf, cfg, "attention1d", "linear", True)
    (ref * tgt).sum().backward()
    # HIP
    enc = enc.to(DEV)
    got = enc(ids.to(DEV))
    (got * tgt.to(DEV)).sum().backward()
    cs = torch.nn.functional.cosine_similarity(got.detach().cpu(), ref.detach(), dim=-1)
    assert cs.min() > 0.999, cs
    assert cos_sim(enc.pooling.layer.weight.grad.cpu(), leaf["pooling.layer.weight"].grad) > 0.99
    assert abs(enc.pooling.layer.bias.grad.item() - leaf["pooling.layer.bias"].grad.item()) < 2e-2 * (abs(leaf["pooling.layer.bias"].grad.item()) + 1e-3)
    # d loss / d log_logit_scale = sum_b features_b . tgt_b: three terms of magnitude |features_b| |tgt_b| ~ 14.29 x 8 each that largely cancel (here
    # to ~6.8), so the tolerance is stated on the terms, not on the cancelled sum: 1e-3 relative feature error (the bf16 compute path's level; the
    # feature cosine gate above allows 4.5e-2)
    gs, rs_ = enc.norm[1].log_logit_scale.grad.item(), leaf["norm.1.log_logit_scale"].grad.item()
    term_scale = float((ref.detach().norm(dim=-1) * tgt.norm(dim=-1)).sum())
    assert abs(gs - rs_) < 1e-3 * term_scale, (gs, rs_, term_scale)
    assert cos_sim(enc.proj[1].weight.grad.cpu(), leaf["proj.1.weight"].grad) > 0.999
    if frozen:
        assert enc.transformer.flat.grad is None
    else:
        gq = enc.transformer.view("encoder.layer.0.attention.self.value.weight", enc.transformer.flat.grad).cpu()
        assert cos_sim(gq, leaf["transformer.encoder.layer.0.attention.self.value.weight"].grad) > 0.99
        ge = enc.transformer.view("encoder.emb_layer_norm_after.weight", enc.transformer.flat.grad).cpu()
        assert cos_sim(ge, leaf["transformer.encoder.emb_layer_norm_after.weight"].grad) > 0.99


def test_struct_encoder_adapter_vs_reference(golden_dir):
    """StructEncoder (pocket / struct_graph modality, ref struct_graph_encoder.py:5-42): the opaque encoder runs under torch autograd, the head /
    normalisation / logit scale on the HIP kernels; features and EVERY gradient (opaque module, head, learnable logit scale) vs the reference's
    own run (tests/golden/struct_graph.pt), and a CLIP sub-step through OneProtLitModule with the modality named `pocket`."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.struct_graph_encoder import StructEncoder
    cases = torch.load(os.path.join(golden_dir, "struct_graph.pt"), weights_only=False)
    for name, c in cases.items():
        D = c["D"]
        opaque = torch.nn.Sequential(torch.nn.Linear(12, 40), torch.nn.Tanh(), torch.nn.Linear(40, D))
        enc = StructEncoder(opaque, output_dim=D, proj_type=c["proj_type"], use_logit_scale=c["use_logit_scale"], learnable_logit_scale=c["learnable"], dropout=0.25)
        enc.load_state_dict(c["sd"], strict=True)
        enc = enc.to(DEV).eval()
        feat = enc(c["batch"].to(DEV))
        (feat * c["tgt"].to(DEV)).sum().backward()
        assert (feat.detach().cpu() - c["features"]).abs().max() < 1e-4 * max(1.0, float(c["features"].abs().max())), name
        got = {n: p.grad.detach().cpu() for n, p in enc.named_parameters() if p.grad is not None}
        assert set(got) == set(c["grads"]), (name, set(got) ^ set(c["grads"]))
        for k, r in c["grads"].items():
            assert (got[k] - r).abs().max() < 2e-4 * max(1.0, float(r.abs().max())) + 1e-6, (name, k, float((got[k] - r).abs().max()), float(r.abs().max()))
    # through the module: sequence <-> pocket sub-step (the 4th modality of cfg-5), head + opaque encoder train, loss finite and decreasing
    from src.models.components.sequence_encoder import SequenceEncoder
    from src.models.oneprot_module import OneProtLitModule
    from oneprot_amd.optim import FusedAdam
    torch.manual_seed(9)
    seq = SequenceEncoder("facebook/esm2_t6_8M_UR50D", output_dim=64, pooling_type="mean", proj_type="linear", use_lora=False, frozen=True)
    pocket = StructEncoder(torch.nn.Sequential(torch.nn.Linear(12, 40), torch.nn.Tanh(), torch.nn.Linear(40, 64)), output_dim=64, proj_type="linear", use_logit_scale=True, dropout=0.0)
    module = OneProtLitModule(components={"sequence": seq, "pocket": pocket}, optimizer=functools.partial(torch.optim.Adam, lr=1e-2), loss_fn="CLIP",
                              use_l1_regularization=True).to(DEV)
    gen = torch.Generator().manual_seed(4)
    ids = torch.randint(4, 24, (8, 32), generator=gen); ids[:, 0] = 0; ids[:, -1] = 2
    graph = torch.randn(8, 12, generator=gen)
    batch = {"pocket": (ids.to(DEV), graph.to(DEV), "pocket", None)}
    losses = [float(module.training_step(batch, i).detach()) for i in range(6)]
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0], losses


def test_arena_gradient_buffer_is_not_recycled_under_a_live_reference(tmp_path):
    """The arena gradient lives in one persistent buffer per encoder (stable addresses for RCCL) that the next backward zero-fills.  A caller that
    still holds last step's gradient (`g = p.grad` across `zero_grad(set_to_none=True)`) must keep its values: the next backward then takes a fresh
    tensor; with no outside reference the buffer is reused."""
    os.environ.update(RANK="0", WORLD_SIZE="1", ONEPROT_ALLOW_RANDOM_INIT="1")
    from src.models.components.sequence_encoder import SequenceEncoder
    cfg = dict(vocab=33, hidden=64, layers=2, heads=4, ffn=128, pad=1, mask=32, eps=1e-5)
    torch.manual_seed(11)
    enc = SequenceEncoder(esm_dir_from_cfg(str(tmp_path), cfg, "esm64"), output_dim=16, pooling_type="mean", proj_type="linear", use_lora=False, frozen=False).to(DEV)
    ids = torch.randint(4, 24, (3, 19), generator=torch.Generator().manual_seed(3)).to(DEV)
    flat = enc.transformer.flat
    enc(ids).sum().backward()
    kept = flat.grad                                   # somebody keeps last step's gradient
    snap, ptr = kept.clone(), kept.data_ptr()
    assert float(snap.abs().sum()) > 0
    enc.zero_grad(set_to_none=True)
    (enc(ids) * 2).sum().backward()
    assert torch.equal(kept, snap), "the kept gradient was overwritten by the next backward"
    assert flat.grad.data_ptr() != ptr
    assert torch.allclose(flat.grad, 2 * snap, rtol=2e-2, atol=1e-4 * float(snap.abs().max()))
    del kept
    enc.zero_grad(set_to_none=True)
    enc(ids).sum().backward()
    p1 = flat.grad.data_ptr()
    enc.zero_grad(set_to_none=True)
    enc(ids).sum().backward()
    assert flat.grad.data_ptr() == p1, "without an outside reference the persistent buffer is reused"
