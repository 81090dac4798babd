"""CPU restatement of the joint CTC/attention objective of a hybrid model (include/masr.h masr_create_ctc) on the oracle (oracle.ref_cpu).

    loss = (1 - w) * L_att + w * L_ctc
    L_att  the decoder's label-smoothed CE of ref_cpu.run_batch_train, unchanged
    L_ctc  nn.CTCLoss(blank=0, reduction='mean', zero_infinity=True) of log_softmax(ctc.ctc_lo(memory)) laid out [T', B, odim];
           memory = the encoder's final LayerNorm output (no dropout), targets = the labels y (no sos / eos), input lengths
           enc_lens = floor(ilens / 4), target lengths = olens as the caller passes them

Gradients come from autograd on leafified params; under ref_cpu.bf16_emulation() the head reads the bf16-rounded memory and weight,
as the engine's GEMM does (fp32 accumulation, fp32 logits)."""
import torch
import torch.nn.functional as F

from oracle import ref_cpu

HEAD = ("ctc.ctc_lo.weight", "ctc.ctc_lo.bias")


def with_head(sd, odim, seed):
    """sd plus a seeded CTC head (scaled like xavier_uniform_ / Linear's bias init), appended behind every other tensor"""
    E = sd["vgg2enc.weight"].shape[0]
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    a = (6.0 / (E + odim)) ** 0.5
    out[HEAD[0]] = (torch.rand(odim, E, generator=g) * 2 - 1) * a
    out[HEAD[1]] = (torch.rand(odim, generator=g) * 2 - 1) / E ** 0.5
    return out


def leafify(sd, cfg):
    p = ref_cpu.leafify({k: v for k, v in sd.items() if k not in HEAD}, cfg)
    for k in HEAD:
        p[k] = sd[k].detach().clone().requires_grad_(True)
    return p


def ctc_log_probs(p, cfg, xs_pad, ilens):
    """log_softmax of the head over the encoder memory -> ([T', B, odim], enc_lens)"""
    enc, enc_lens = ref_cpu.extract_feat(p, xs_pad, ilens)
    enc = enc.transpose(0, 1)
    enc = enc + p["pos_encoder.pe"][:enc.shape[0]]
    memory = ref_cpu.encoder_forward(p, cfg, enc, ref_cpu.make_bool_pad_mask(enc_lens))
    z = ref_cpu._q(memory) @ ref_cpu._q(p[HEAD[0]]).t() + p[HEAD[1]]
    return torch.log_softmax(z, dim=-1), enc_lens


def ctc_term(p, cfg, xs_pad, ilens, ys, olens):
    lp, enc_lens = ctc_log_probs(p, cfg, xs_pad, ilens)
    tgt = torch.cat([torch.as_tensor(y, dtype=torch.int64).reshape(-1) for y in ys])
    loss = F.ctc_loss(lp, tgt, enc_lens, torch.as_tensor(olens, dtype=torch.int64), blank=0, reduction="mean", zero_infinity=True)
    return loss, lp


def run_batch_train(p, cfg, batch, eps, w):
    """forward + joint loss + backward -> (info, {name: grad}) with the head's gradients included; `batch` as ref_cpu.run_batch_train's
    (its olens are left untouched here)"""
    xs_pad, ilens, ys, olens = batch
    names = ref_cpu.grad_param_names({k: v for k, v in p.items() if k not in HEAD}, cfg) + list(HEAD)
    for n in names:
        p[n].grad = None
    logit, gold = ref_cpu.model_forward(p, cfg, xs_pad, ilens, ys, olens.clone())
    l_att, n_correct, n_total = ref_cpu.label_smoothed_ce(logit, gold, eps)
    l_ctc, _ = ctc_term(p, cfg, xs_pad, ilens, ys, olens)
    loss = (1.0 - w) * l_att + w * l_ctc
    loss.backward()
    grads = {n: p[n].grad for n in names}
    info = {"loss": float(loss.detach()), "att": float(l_att.detach()), "ctc": float(l_ctc.detach()), "acc": float(n_correct) / n_total}
    return info, grads


def inner_step(p, cfg, batch, eps, w, bufs, lr, momentum=0.9, nesterov=True):
    """one inner step (run_batch -> clip 5 -> SGD nesterov) of the joint objective, as ref_cpu.inner_step"""
    info, grads = run_batch_train(p, cfg, batch, eps, w)
    gn = ref_cpu.clip_grad_norm_(grads)
    ref_cpu.sgd_nesterov_step(p, grads, bufs, lr, momentum, nesterov)
    info["grad_norm"] = gn
    return info
