"""Shared by tests/test_slot_layout_cpu.py and the GPU tie-in test: the library's host-only slot-layout entry (bnmtf_slot_layout:
what bnmtf_create builds for one direction from the units' missing inner indices; csrc/slot_layout.hip) behind a NumPy face."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from bnmtf_amd import _lib

INFO = ("mz", "pw", "nch", "mh", "pw_chunk", "pw1", "pair_ok", "wide_can", "use_wide", "use_turns", "use_twin", "f_nw", "vb_path",
        "uw_ok", "u_nw", "ho_ppb", "stats_blocks", "npairs", "emax", "slots", "u_emax")
TABLES = (("unit_map", np.int32), ("pair_E", np.uint32), ("pair_base", np.uint32), ("off", np.uint32), ("off16", np.uint32),
          ("gen_units", np.int32), ("row_blk", np.uint16), ("u_unit_map", np.int32), ("u_pair_E", np.uint32),
          ("u_pair_base", np.uint32), ("u_off16", np.uint32))
INFO_LEN = 32       # BNMTF_SLOT_INFO_LEN


def missing_lists(miss):
    """CSR (ptr [n + 1], idx) of the True entries of the boolean matrix miss [n][m]: every unit's missing inner indices, ascending."""
    miss = np.asarray(miss, dtype=bool)
    ptr = np.zeros(miss.shape[0] + 1, dtype=np.uint32)
    ptr[1:] = np.cumsum(miss.sum(axis=1))
    return ptr, np.nonzero(miss)[1].astype(np.uint32)


def raw_call(n, m, KP, world, ptr, idx, info, tables):
    return _lib.lib().bnmtf_slot_layout(int(n), int(m), int(KP), int(world), _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(info),
                                        *[_lib.ptr(t) for t in tables])


def slot_layout(miss, KP=32, world=1):
    """The layout of the units whose missing entries are the True entries of miss [n][m]: a namespace of the scalars (INFO), the
    tables (TABLES; off / off16 as [rows][64], the others flat) and `sizes`.  Two calls: the sizes, then the tables."""
    miss = np.asarray(miss, dtype=bool)
    n, m = miss.shape
    ptr, idx = missing_lists(miss)
    info = np.zeros(INFO_LEN, dtype=np.int64)
    _lib.check(raw_call(n, m, KP, world, ptr, idx, info, [None] * len(TABLES)))
    sizes = info[len(INFO):].copy()
    assert len(INFO) + len(TABLES) == INFO_LEN
    tables = [np.zeros(int(s), dtype=dt) for (_, dt), s in zip(TABLES, sizes)]
    info2 = np.zeros(INFO_LEN, dtype=np.int64)
    _lib.check(raw_call(n, m, KP, world, ptr, idx, info2, tables))
    assert (info == info2).all()
    out = SimpleNamespace(n=n, m=m, KP=KP, sizes=dict(zip([t for t, _ in TABLES], map(int, sizes))),
                          **{k: int(v) for k, v in zip(INFO, info)}, **{name: t for (name, _), t in zip(TABLES, tables)})
    for name in ("off", "off16", "u_off16"):
        setattr(out, name, getattr(out, name).reshape(-1, 64))
    return out


def random_missing(rs, n, m, frac):
    """[n][m] booleans, each True with probability frac -- but never a whole row (bnmtf_create refuses an unobserved unit)."""
    miss = rs.uniform(size=(n, m)) < frac
    miss[np.arange(n), rs.randint(0, m, n)] = False
    return miss
