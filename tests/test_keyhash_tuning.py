"""GroupByKeyHash is validated like WordCountKernel and carried by tuning.from_ctx (ops/tuning.py)."""
import pytest

import dryad_amd as D
from dryad_amd.ops import tuning


@pytest.mark.parametrize("value", ["off", "on", "auto"])
def test_groupby_keyhash_is_carried(value):
    ctx = D.DryadLinqContext(1)
    assert tuning.from_ctx(ctx).groupby_keyhash == tuning.Tuning().groupby_keyhash
    ctx.GroupByKeyHash = value
    assert tuning.from_ctx(ctx).groupby_keyhash == value
    with tuning.scope(ctx):
        assert tuning.current().groupby_keyhash == value


def test_groupby_keyhash_rejects_other_values():
    ctx = D.DryadLinqContext(1)
    ctx.GroupByKeyHash = "hash"
    with pytest.raises(ValueError, match="GroupByKeyHash"):
        tuning.from_ctx(ctx)
