"""WordCountKernel is validated like GroupByMatrix and carried by tuning.from_ctx (ops/tuning.py)."""
import pytest

import dryad_amd as D
from dryad_amd.ops import tuning


@pytest.mark.parametrize("value", ["auto", "hash", "sort"])
def test_wordcount_kernel_is_carried(value):
    ctx = D.DryadLinqContext(1)
    assert tuning.from_ctx(ctx).wordcount_kernel == tuning.Tuning().wordcount_kernel
    ctx.WordCountKernel = value
    assert tuning.from_ctx(ctx).wordcount_kernel == value
    with tuning.scope(ctx):
        assert tuning.current().wordcount_kernel == value


def test_wordcount_kernel_rejects_other_values():
    ctx = D.DryadLinqContext(1)
    ctx.WordCountKernel = "radix"
    with pytest.raises(ValueError, match="WordCountKernel"):
        tuning.from_ctx(ctx)
