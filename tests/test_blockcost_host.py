"""cp.quotientpattern exists on the HIP backend only: any other backend is refused by name, as permute is (no GPU needed)."""
import numpy as np
import pytest

from util import cp, sprand


def test_quotientpattern_names_the_backend_it_refuses(orc):
    A = sprand(8, 16, 0.3, np.random.default_rng(0))
    Pi = cp.SplitPartition(2, [1, 5, 9])
    with pytest.raises(NotImplementedError, match="backend 'oracle'"):
        cp.quotientpattern(A, Pi, backend=orc)
