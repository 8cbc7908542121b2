"""Per-job operator strategy choices, taken from context properties (no import-time environment
knobs in the kernel library): the GPU executor enters ``scope(ctx)`` for each job on its job
thread, and operators read ``current()``.  Outside a job the defaults apply.

    GroupByAggregation   "auto" | "radix" | "sort": radix-partitioned LDS aggregation for a
                         single integer key (ops/radixagg.py) only for keys spanning >= 2^32
                         values ("auto"), for every large integer key ("radix"), or never ("sort").
    GroupByMatrix        "off" | "on": a GroupBy of one integer key whose sample shows <= 256 distinct
                         keys, with integer Count / Sum / Min / Max only, tries the exact int8
                         one-hot MFMA aggregation (ops/matagg.py, csrc/kernels/matagg.hip) before
                         the LDS hash tables.  "off" by default: at 1e9 rows it is 1.6x faster than
                         the hash tables with 16 keys, level at 64 and 2.8x slower at 256
                         (profiles/matagg_bw.log).
    WordCountKernel      "auto" | "hash" | "sort": the word counts of a text partition (ops/text.py) from
                         the fused tokenise-and-count pass with LDS hash tables (ops/wordcount.py,
                         csrc/kernels/wordcount.hip) first ("auto", "hash": the sort path only when its
                         table overflows or two words share a tag), or always by sorting token hashes.
                         "auto" by default: on 1 GB of the benchmark's 50 000-word Zipf text the call
                         takes 10.8 ms against 52.4 ms and the job step 56 ms against 97 ms; a text
                         with more than 2^21 distinct words pays 10 ms for the pass that overflows
                         (profiles/wordcount_bw.log, profiles/wordcount_job.log).
    GroupByKeyHash       "off" | "on" | "auto": a GroupBy whose key is a string, a tuple of columns (with
                         or without string parts) or wider than one sort entry, and a Distinct over
                         records with string fields, try the tag-and-verify hash aggregation with LDS
                         tables (ops/keyhash.py, csrc/kernels/keyhash.hip) before the fingerprint sort
                         ("on"; "auto": only on >= 2^16 rows whose sampled distinct estimate is below
                         half the rows).  "off" by default: the call is faster than the sort branch
                         (1e8 rows of gen://names keys, 1e3 names: 19.3 ms against 33.0 ms, 1e5 names:
                         27.9 against 47.3 ms; an (int64, int32) key, 1e9 rows, 1e3 pairs: 185 against
                         237 ms) and so is the job step for a string key (89 ms against 99 ms), but the
                         job step for a composite key is not measured (profiles/keyhash_bw.log).
    TopKMinRows          OrderBy(...).Take(k) over at least this many rows of one partition ...
    TopKMaxFraction      ... with k <= rows * fraction runs as a radix select of the k smallest
                         sort entries (ops/topk.py) instead of a full sort and a slice.
"""
from __future__ import annotations

import contextlib
import contextvars
from dataclasses import dataclass, replace


@dataclass(frozen=True)
class Tuning:
    groupby_aggregation: str = "auto"
    groupby_matrix: str = "off"
    wordcount_kernel: str = "auto"
    groupby_keyhash: str = "off"
    topk_min_rows: int = 1 << 24
    topk_max_fraction: float = 1 / 8


_CUR: contextvars.ContextVar = contextvars.ContextVar("dryad_tuning", default=Tuning())


def current() -> Tuning:
    return _CUR.get()


def from_ctx(ctx) -> Tuning:
    props = ctx._props if ctx is not None else {}
    agg = props.get("GroupByAggregation") or "auto"
    if agg not in ("auto", "radix", "sort"):
        raise ValueError(f"GroupByAggregation must be auto, radix or sort, not {agg!r}")
    mat = props.get("GroupByMatrix") or "off"
    if mat not in ("off", "on"):
        raise ValueError(f"GroupByMatrix must be off or on, not {mat!r}")
    t = Tuning()
    wc = props.get("WordCountKernel") or t.wordcount_kernel
    if wc not in ("auto", "hash", "sort"):
        raise ValueError(f"WordCountKernel must be auto, hash or sort, not {wc!r}")
    kh = props.get("GroupByKeyHash") or t.groupby_keyhash
    if kh not in ("off", "on", "auto"):
        raise ValueError(f"GroupByKeyHash must be off, on or auto, not {kh!r}")
    rows, frac = props.get("TopKMinRows"), props.get("TopKMaxFraction")
    return replace(t, groupby_aggregation=agg, groupby_matrix=mat, wordcount_kernel=wc, groupby_keyhash=kh,
                   topk_min_rows=t.topk_min_rows if rows is None else int(rows),
                   topk_max_fraction=t.topk_max_fraction if frac is None else float(frac))


@contextlib.contextmanager
def scope(ctx=None, **kw):
    t = replace(from_ctx(ctx), **kw) if ctx is not None else replace(current(), **kw)
    tok = _CUR.set(t)
    try:
        yield t
    finally:
        _CUR.reset(tok)
