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
    rows, frac = props.get("TopKMinRows"), props.get("TopKMaxFraction")
    return replace(t, groupby_aggregation=agg, groupby_matrix=mat,
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
