"""Device string sort throughput (ops/strsort.sort_strings, csrc/kernels/strsort.hip):

    python tools/micro/strsort_bw.py [strings] [host_strings]

Sorts ``strings`` (default 1e8) generated printable-ASCII strings of 16..32 bytes, in two
distributions: distinct random tails (the first window decides almost every string) and a shared
24-byte prefix (three window passes over everything before the bytes differ).  Prints the best of
3 sorts in ms (host clock around the call, which ends in a device synchronise) and GB/s of heap
bytes.  The same input at ``host_strings`` rows (default 1e6) is also sorted the way the GPU
executor's host fallback does it (table -> Python strings -> sorted -> table), checked against the
device permutation."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import torch  # noqa: E402

from dryad_amd.gpu.table import from_objects, text_table  # noqa: E402
from dryad_amd.ops.strsort import sort_strings  # noqa: E402

PREFIX = b"tenant-0042/events/2026/"          # 24 bytes
CHUNK = 1 << 22


def generate(n, shared_prefix, seed=1):
    """(heap, off, len) of n strings; with ``shared_prefix`` every string starts with PREFIX (cut
    to the string's length).  The heap is built in pieces of CHUNK strings, so every index used
    is local to a small piece and masked to its own string."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    ln = torch.randint(16, 33, (n,), dtype=torch.int64, device="cuda", generator=g)
    off = torch.cumsum(ln, 0) - ln
    heap = torch.empty(int(ln.sum()), dtype=torch.uint8, device="cuda")
    pre = torch.tensor(list(PREFIX), dtype=torch.uint8, device="cuda")
    k = torch.arange(len(PREFIX), device="cuda")
    for a in range(0, n, CHUNK):
        b = min(n, a + CHUNK)
        lo, hi = int(off[a]), int(off[b - 1] + ln[b - 1])
        piece = torch.randint(0x20, 0x7F, (hi - lo,), dtype=torch.uint8, device="cuda", generator=g)
        if shared_prefix:
            inside = k[None, :] < ln[a:b, None]                  # never past the string's end
            idx = (off[a:b, None] - lo) + k[None, :]
            piece[idx[inside]] = pre.expand(b - a, -1)[inside]
        heap[lo:hi] = piece
    return heap, off, ln


def timed(fn, reps=3):
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def host_fallback(heap, off, ln):
    """The executor's host path for a sort it cannot trace: device table -> Python strings ->
    sorted -> device table."""
    t0 = time.perf_counter()
    strs = text_table(heap, off, ln, str).to_objects()
    out = from_objects(sorted(strs), None, heap.device)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, strs, out


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
    nh = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1_000_000
    for name, shared in (("distinct random tails", False), ("shared 24-byte prefix", True)):
        for rows, host in ((nh, True), (n, False)):
            heap, off, ln = generate(rows, shared)
            perm = sort_strings(heap, off, ln)             # warm-up: code objects, workspaces
            ms = timed(lambda: sort_strings(heap, off, ln))
            print(f"{name}: {rows} strings, {heap.numel() / 1e9:.3f} GB heap: sort_strings {ms:.2f} ms = "
                  f"{heap.numel() / 1e6 / ms:.1f} GB/s", flush=True)
            if host:
                hms, strs, _ = host_fallback(heap, off, ln)
                assert perm.tolist() == sorted(range(rows), key=strs.__getitem__), "device order != Python order"
                print(f"{name}: {rows} strings: host fallback {hms:.0f} ms ({hms / ms:.0f}x the device sort), "
                      f"orders equal", flush=True)
            del heap, off, ln, perm


if __name__ == "__main__":
    main()
