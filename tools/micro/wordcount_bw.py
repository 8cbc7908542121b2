"""WordCount of one text partition: the fused LDS hash-table kernels against the token sort
(ops/text.word_count_table with WordCountKernel "hash" / "sort"; csrc/kernels/wordcount.hip):

    python tools/micro/wordcount_bw.py [bytes]

``bytes`` (default 1e9) of text are built in HBM from a seed, no files, for three vocabularies:
the benchmark's 50 000 random words with Zipf(1.3) ranks (models/wordcount.synthetic_corpus), 5e6
words drawn uniformly (more than the hash path's global table takes at its default capacity) and
all tokens distinct (the same, so both measure the hash pass wasted in front of the sort path).
The two settings are called alternately in one process: min and max of 3 timed calls each after
a warm-up, host clock around a call that ends in a device synchronise.  The two tables are
compared as dictionaries on the device (words padded to 16 bytes, sorted with their counts).
GB/s is the text over the call's time; the hash path reads the text twice (count, verify), so
2n / time stands next to the 2n / time of a ``copy_`` of the same buffer."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dryad_amd.ops import text as TX  # noqa: E402
from dryad_amd.ops import tuning  # noqa: E402
from dryad_amd.ops import wordcount as WC  # noqa: E402

DEV = "cuda"


def call_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def letters(idx: torch.Tensor, width: int) -> torch.Tensor:
    """[len(idx), width] uint8: idx in base 26 as lower-case letters."""
    p = 26 ** torch.arange(width, device=DEV, dtype=torch.int64)
    return (idx[:, None] // p % 26 + 97).to(torch.uint8)


def zipf_vocabulary(vocab=50_000, seed=1):
    """The words of synthetic_corpus and the cumulative distribution of min(zipf(1.3) - 1, vocab - 1)."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    words = [alphabet[rng.integers(0, 26, size=int(rng.integers(2, 10)))] for _ in range(vocab)]
    wlen = torch.tensor([len(w) for w in words], dtype=torch.int64, device=DEV)
    heap = torch.from_numpy(np.concatenate(words)).to(DEV)
    k = np.arange(1, 2_000_001, dtype=np.float64)
    zeta = (k ** -1.3).sum() + k[-1] ** -0.3 / 0.3 - 0.5 * k[-1] ** -1.3      # Euler-Maclaurin tail
    cdf = np.cumsum(k[:vocab - 1] ** -1.3 / zeta)
    return heap, torch.cumsum(wlen, 0) - wlen, wlen, torch.from_numpy(cdf).to(DEV)


def text_of(ranks, heap, wstart, wlen, first_token):
    """The words ``ranks`` joined by ' ', every 12th by '\\n', with one after the last."""
    ln1 = wlen[ranks] + 1
    ends = torch.cumsum(ln1, 0)
    tok = torch.repeat_interleave(torch.arange(ranks.numel(), device=DEV), ln1)
    rel = torch.arange(int(ends[-1]), device=DEV) - (ends - ln1)[tok]
    inside = rel < wlen[ranks][tok]
    out = heap[torch.where(inside, wstart[ranks][tok] + rel, 0)]
    sep = torch.where((tok + first_token) % 12 == 11, 10, 32).to(torch.uint8)
    return torch.where(inside, out, sep)


def build(kind: str, n: int, gen) -> torch.Tensor:
    if kind == "distinct":                      # token i is i in base 26, 6 letters for up to 3e8 tokens
        m = n // 7
        t = torch.full((m, 7), 32, dtype=torch.uint8, device=DEV)
        t[:, :6] = letters(torch.arange(m, device=DEV), 6)
        t[11::12, 6] = 10
        return t.flatten()
    if kind == "zipf":
        heap, wstart, wlen, cdf = zipf_vocabulary()
    else:
        V = 5_000_000
        heap = letters(torch.arange(V, device=DEV), 5).flatten()
        wlen = torch.full((V,), 5, dtype=torch.int64, device=DEV)
        wstart = torch.arange(V, device=DEV) * 5
    parts, have, ntok, step = [], 0, 0, 8_000_000
    while have < n:
        if kind == "zipf":
            ranks = torch.searchsorted(cdf, torch.rand(step, device=DEV, dtype=torch.float64, generator=gen))
        else:
            ranks = torch.randint(0, wlen.numel(), (step,), device=DEV, generator=gen)
        parts.append(text_of(ranks, heap, wstart, wlen, ntok))
        have += parts[-1].numel()
        ntok += step
    t = torch.cat(parts)[:n].clone()
    t[-1] = 10
    return t


def as_sorted_dict(t):
    """(words as [g, 2] int64 of their zero-padded 16 bytes, counts), sorted by word."""
    off, ln, cnt = t.cols["Item1"], t.cols["Item1#len"], t.cols["Item2"].to(torch.int64)
    assert int(ln.max()) <= 16
    j = torch.arange(16, device=DEV)
    b = t.strs["Item1"][(off[:, None] + j).clamp_max(t.strs["Item1"].numel() - 1)]
    w = torch.where(j < ln[:, None], b, 0).to(torch.uint8).contiguous().view(torch.int64)
    o = torch.argsort(w[:, 1], stable=True)
    o = o[torch.argsort(w[o, 0], stable=True)]
    return w[o], cnt[o]


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
    gen = torch.Generator(device=DEV).manual_seed(7)
    for kind in ("zipf", "5e6", "distinct"):
        buf = build(kind, n, gen)
        dst = torch.empty_like(buf)
        cp = min(call_ms(lambda: dst.copy_(buf))[0] for _ in range(4))
        del dst
        ms, out, path, wc = {"sort": [], "hash": []}, {}, {}, {}
        for rep in range(4):                           # rep 0 warms both up
            for k in ms:
                with tuning.scope(wordcount_kernel=k):
                    t, r = call_ms(lambda: TX.word_count_table(buf))
                path[k] = TX.stats["path"]
                if k == "hash":
                    wc = dict(WC.stats)
                if rep == 3:
                    out[k] = as_sorted_dict(r)
                del r
                if rep:
                    ms[k].append(t)
        same = all(torch.equal(a, b) for a, b in zip(out["sort"], out["hash"]))
        assert same, f"{kind}: the two tables differ"
        s, h = ms["sort"], ms["hash"]
        print(f"{kind}: n = {n}, {out['sort'][1].numel()} words: "
              f"sort {min(s):.2f} .. {max(s):.2f} ms ({n / min(s) / 1e6:.1f} GB/s of text); "
              f"hash {min(h):.2f} .. {max(h):.2f} ms ({n / min(h) / 1e6:.1f} GB/s of text, path {path['hash']}, "
              f"flushes {wc['flushes']}, overflow {wc['overflow']}), 2n / time {2 * n / min(h) / 1e6:.0f} GB/s "
              f"against copy_ {2 * n / cp / 1e6:.0f} GB/s; sort / hash {min(s) / min(h):.2f}x; tables equal",
              flush=True)
        del buf, out


if __name__ == "__main__":
    main()
