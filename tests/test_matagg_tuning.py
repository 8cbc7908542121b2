"""GroupByMatrix is validated like GroupByAggregation (ops/tuning.py)."""
import pytest

import dryad_amd as D
from dryad_amd.ops import tuning


def test_groupby_matrix_rejects_other_values():
    ctx = D.DryadLinqContext(1)
    assert tuning.from_ctx(ctx).groupby_matrix == "off"
    ctx.GroupByMatrix = "maybe"
    with pytest.raises(ValueError, match="GroupByMatrix"):
        tuning.from_ctx(ctx)
