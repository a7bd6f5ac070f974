"""The layout bnmtf_create built on the device's missing lists is the one bnmtf_slot_layout builds from the same mask on the
host (csrc/slot_layout.hip; tests/test_slot_layout_cpu.py checks that one's tables): what describe() says of both directions
against the entry's scalars, for the unit / pair-layout case 192 x 130, K = 12, half of the entries missing."""
import re

import numpy as np
import pytest

from _slot_layout import random_missing, slot_layout
from bnmtf_amd import bnmf_gibbs_optimised

pytestmark = pytest.mark.gpu

PRI = dict(alpha=1., beta=1., lambdaU=0.1, lambdaV=0.1)
I, J, K = 192, 130, 12


def _said(desc, which):
    return dict(kv.split("=") for kv in re.search(r"%s\[([^\]]*)\]" % which, desc).group(1).split())


@pytest.mark.parametrize("env", [{}, {"BNMTF_UNIT": "0"}], ids=["unit", "pairs"])
def test_describe_agrees_with_the_host_entry(monkeypatch, env):
    rs = np.random.RandomState(192130)
    miss = random_missing(rs, I, J, 0.5)
    miss[rs.randint(0, I, J), np.arange(J)] = False              # no unobserved column either
    R = rs.exponential(1.0, (I, K)) @ rs.exponential(1.0, (J, K)).T
    monkeypatch.setenv("BNMTF_SMALL", "0")                        # the dense layout, built by bnmtf_create itself
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    b = bnmf_gibbs_optimised(R, (~miss).astype(np.float64), K, PRI, verbose=False, seed=3)
    desc = b.describe()
    b.close()
    assert "handover=0" in desc, desc                             # (so unit_sweep's first figure is the layout's uw_ok)
    unit = re.search(r"unit_sweep\[rows=(\d+)/(\d+)/(\d+) cols=(\d+)/(\d+)/(\d+)\]", desc).groups()
    for which, mk, triple in (("rows", miss, unit[:3]), ("cols", miss.T, unit[3:])):
        L = slot_layout(np.ascontiguousarray(mk), KP=32)
        said = _said(desc, which)
        nslots = int(((mk.sum(axis=1) + 63) // 64 * 64).sum())    # the generic kernel's 64-wide slots of the lists the entry was given
        assert (int(said["nslots"]), int(said["sweep_nw"]), int(said["emax"]), int(said["generic_units"])) == \
            (nslots, L.f_nw, L.emax, L.sizes["gen_units"]), (which, desc)
        assert tuple(map(int, triple)) == (L.uw_ok, L.u_nw, L.u_emax), (which, desc)
        assert L.uw_ok == (0 if env else 1)
