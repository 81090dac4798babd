"""Train the LSTM LM that `--decode_mode nlm_beam` reads (masr_amd/nlm.py): Embedding -> LSTM -> Linear over the model's output
units, with stock torch.nn, on a text file of unit-id lines (one sentence per line, space-separated ids in [1, C - 2], as the right-hand
column of best-hyp or the labels of a shard).  Input [sos] + sentence, target sentence + [eos]; sos = 0 and eos = C - 1 (--start eos trains
with eos in front instead, for `beam_decode.lm_start: eos`).  Saves the state dict in this project's key layout (embed.weight, rnn.*, lo.*).
A tool: nothing in the package imports it and it is on no measured path.
usage: python tools/train_nlm.py TEXT OUT.pt --classes C [--embed 650] [--hidden 650] [--layers 2] [--epochs 10] [--batch 32] [--lr 1e-3]
                                 [--dropout 0.0] [--start sos|eos] [--device cpu] [--seed 531]"""
import argparse
import math

import torch


class LstmLMModule(torch.nn.Module):
    def __init__(self, C, E, H, L, dropout=0.0):
        super().__init__()
        self.embed = torch.nn.Embedding(C, E)
        self.rnn = torch.nn.LSTM(E, H, L, dropout=dropout if L > 1 else 0.0)
        self.lo = torch.nn.Linear(H, C)

    def forward(self, tokens):                                  # [T, B] -> [T, B, C]
        return self.lo(self.rnn(self.embed(tokens))[0])


def read_sentences(path, C):
    out = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            ids = [int(w) for w in line.split()]
            if any(not 1 <= i <= C - 2 for i in ids):
                raise ValueError(f"{path}: line {no}: unit ids must lie in [1, {C - 2}]")
            if ids:
                out.append(ids)
    if not out:
        raise ValueError(f"{path}: no sentences")
    return out


def batches(sents, bs, start, eos, gen):
    order = torch.randperm(len(sents), generator=gen).tolist()
    for i in range(0, len(order), bs):
        chunk = [sents[j] for j in order[i:i + bs]]
        T = max(len(s) for s in chunk) + 1
        x = torch.full((T, len(chunk)), eos, dtype=torch.long)
        y = torch.full((T, len(chunk)), -100, dtype=torch.long)
        for b, s in enumerate(chunk):
            x[:len(s) + 1, b] = torch.tensor([start] + s)
            y[:len(s) + 1, b] = torch.tensor(s + [eos])
        yield x, y


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("text"); ap.add_argument("out")
    ap.add_argument("--classes", type=int, required=True)
    ap.add_argument("--embed", type=int, default=650); ap.add_argument("--hidden", type=int, default=650); ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--epochs", type=int, default=10); ap.add_argument("--batch", type=int, default=32); ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--dropout", type=float, default=0.0); ap.add_argument("--start", choices=["sos", "eos"], default="sos")
    ap.add_argument("--device", default="cpu"); ap.add_argument("--seed", type=int, default=531)
    a = ap.parse_args()
    C = a.classes
    if not (2 <= C <= 65535 and 1 <= a.embed <= 2048 and 1 <= a.hidden <= 2048 and 1 <= a.layers <= 4):
        raise SystemExit("need 2 <= classes <= 65535, 1 <= embed, hidden <= 2048, 1 <= layers <= 4 (include/masr.h masr_nlm_create)")
    torch.manual_seed(a.seed)
    gen = torch.Generator().manual_seed(a.seed)
    sents = read_sentences(a.text, C)
    model = LstmLMModule(C, a.embed, a.hidden, a.layers, a.dropout).to(a.device)
    opt = torch.optim.Adam(model.parameters(), lr=a.lr)
    start, eos = (0 if a.start == "sos" else C - 1), C - 1
    for ep in range(a.epochs):
        model.train()
        tot, n = 0.0, 0
        for x, y in batches(sents, a.batch, start, eos, gen):
            x, y = x.to(a.device), y.to(a.device)
            loss = torch.nn.functional.cross_entropy(model(x).view(-1, C), y.view(-1), ignore_index=-100, reduction="sum")
            k = int((y >= 0).sum())
            opt.zero_grad()
            (loss / k).backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), 5.0)
            opt.step()
            tot, n = tot + float(loss), n + k
        print(f"epoch {ep + 1}: {tot / n:.4f} nats per token, perplexity {math.exp(tot / n):.2f}", flush=True)
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, a.out)
    print(f"saved {a.out}: {a.layers} x {a.hidden} LSTM on {a.embed}-dim embeddings over {C} classes, start token {a.start}")


if __name__ == "__main__":
    main()
