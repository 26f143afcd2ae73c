"""Fixtures of the edge-band tests (test_edge_band_data_cpu.py, test_edge_bands_*.py): the reference composition and, per test module, the
host side of every pair and shape that the module asks for, built once."""
import pytest

import edge_band_data as D
from matrix8_helpers import m8  # noqa: F401  (fixture: the restatement of CloverMatrix8)


@pytest.fixture(scope="module")
def ref(oracle, m8):  # noqa: F811
    return D.Ref(oracle, m8)


@pytest.fixture(scope="module")
def cases(ref):
    """cases(pair, out, in_) -> edge_band_data.Case"""
    made = {}

    def get(pair, out, in_):
        if (pair, out, in_) not in made:
            made[(pair, out, in_)] = D.Case(ref, pair, out, in_)
        return made[(pair, out, in_)]
    return get
