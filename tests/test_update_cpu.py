"""The sparse row update without a GPU: the entry points in the header, the ctypes table and the library, the host rule (the bit width
of N and the sort's passes: tests/cpu/update_rule_test.cpp), the scratch size, every refusal of legion_row_update
(update_rule.h decides them before any HIP call) and update_rows' ValueErrors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from legion_amd import engine, lib
from tests.rule_table import assert_passes, run_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM, MEAN, SGD, ADAGRAD, ADAM = 0, 1, 0, 1, 2
CAP = 2 ** 22
PTR = ctypes.c_void_p(4096)                                            # not null; m == 0 enqueues nothing, so it is never followed


def test_symbols_in_header_ctypes_table_and_library():
    text = open(os.path.join(ROOT, "include", "legion_hip.h")).read()
    L = lib.load()                                                     # (a name the library does not export fails here)
    for name in ("legion_row_update_scratch_bytes", "legion_row_update"):
        assert re.search(r"\bint(32|64)_t\s+" + name + r"\s*\(", text) and hasattr(L, name), name
    for name, value in (("UPDATE_SGD", SGD), ("UPDATE_ADAGRAD", ADAGRAD), ("UPDATE_ADAM", ADAM), ("ROW_UPDATE_MAX_IDS", CAP)):
        assert re.search(rf"#define\s+LEGION_{name}\s+{value}\b", text), name
    c_p, c_i32, c_i64, c_f32 = lib.c_p, lib.c_i32, lib.c_i64, ctypes.c_float
    assert lib.SIGNATURES["legion_row_update_scratch_bytes"] == (c_i64, [c_i32, c_i32, c_i32])
    assert lib.SIGNATURES["legion_row_update"] == (c_i32, [c_p, c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_i32, c_i32, c_f32, c_f32,
                                                          c_f32, c_f32, c_p, c_p, c_p, c_p, c_i64])
    assert engine.FeatureStorage.OPTIMIZERS == {"sgd": SGD, "adagrad": ADAGRAD, "adam": ADAM} and engine.FeatureStorage.ROW_UPDATE_MAX_IDS == CAP


def test_bits_and_passes_over_a_table(tmp_path):
    """N = 255, 256, 65 536 and 2^24 sort in 1, 2, 3 and 4 passes."""
    assert_passes(run_table(tmp_path, "update_rule"))


def test_scratch_is_monotone_in_m_and_refused_past_the_cap():
    size = lib.load().legion_row_update_scratch_bytes
    for N, D in ((10, 1), (2 ** 24, 128)):
        sizes = [size(m, N, D) for m in (0, 1, 255, 256, 257, 1024, 1025, 2 ** 20, CAP)]
        assert sizes == sorted(sizes) and sizes[0] >= 0 and sizes[-1] > 16 * CAP, (N, D, sizes)
    assert size(CAP, 10, 128) - size(CAP, 10, 1) == (CAP // 128) * 4 * 127, "fewer than m / 128 partial rows of D float32"
    for bad in ((CAP + 1, 10, 4), (-1, 10, 4), (5, 0, 4), (5, 10, 0)):
        assert size(*bad) == -1, bad


REFUSALS = {
    "combine-max": dict(combine=2), "combine-negative": dict(combine=-1), "optimizer": dict(optimizer=3), "optimizer-negative": dict(optimizer=-1),
    "cache-without-map": dict(cache=PTR), "map-without-cache": dict(node_map=PTR), "m": dict(m=-1), "m-past-cap": dict(m=CAP + 1, nbytes=2 ** 40),
    "N": dict(N=0), "D": dict(D=0), "D-negative": dict(D=-4), "null-table": dict(table=None), "null-ids": dict(ids=None),
    "null-grads": dict(grads=None), "null-scratch": dict(scratch=None), "adagrad-state1": dict(optimizer=ADAGRAD, state1=None),
    "adam-state1": dict(optimizer=ADAM, state1=None), "adam-state2": dict(optimizer=ADAM, state2=None),
    "adam-state-pow": dict(optimizer=ADAM, state_pow=None), "scratch-short": dict(nbytes=7), "scratch-negative": dict(nbytes=-1),
    "scratch-short-for-m": dict(m=2 ** 20, nbytes=2 ** 20),
}


def call(L, **change):
    a = dict(table=PTR, cache=None, node_map=None, D=4, N=10, ids=PTR, grads=PTR, m=0, combine=MEAN, optimizer=SGD, state1=PTR, state2=PTR,
             state_pow=PTR, scratch=PTR, nbytes=64)
    a.update(change)
    return L.legion_row_update(None, a["table"], a["cache"], a["node_map"], a["D"], a["N"], a["ids"], a["grads"], a["m"], a["combine"],
                               a["optimizer"], 0.5, 1e-10, 0.9, 0.999, a["state1"], a["state2"], a["state_pow"], a["scratch"], a["nbytes"])


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_every_refusal_returns_minus_one_without_a_device(name):
    L = lib.load()
    assert call(L) == 0, "no ids: accepted, nothing enqueued"
    assert call(L, state1=None, state2=None, state_pow=None) == 0 and call(L, optimizer=ADAGRAD, state2=None, state_pow=None) == 0
    assert call(L, cache=PTR, node_map=PTR, optimizer=ADAM, combine=SUM) == 0
    assert call(L, **REFUSALS[name]) == -1, name


def test_argument_errors_are_value_errors_before_any_device():
    f = engine.FeatureStorage.__new__(engine.FeatureStorage)          # (no handle: the checks come before the library call)
    f._lib, f.float_feature_len, f.total_num_nodes, f.feature_dtype = lib.load(), 4, 10, "float32"
    ids, grads = np.array([1, 2], np.int32), np.zeros((2, 4), np.float32)
    for kw, match in ((dict(optimizer="rmsprop"), "optimizer"), (dict(combine="max"), "combine"), (dict(lr="0.1"), "lr"),
                      (dict(betas=0.9), "betas"), (dict(betas=(0.9, None)), "betas"), (dict(eps=None), "eps"), (dict(state=[]), "state"),
                      (dict(cache=object()), "UnifiedCache"), (dict(dev_id="0"), "dev_id")):
        with pytest.raises(ValueError, match=match):
            f.update_rows(ids, grads, **{"lr": 0.5, **kw})
    with pytest.raises(ValueError, match="int32"):
        f.update_rows(torch.tensor([1, 2]), grads, lr=0.5)
    for bad in (np.zeros((2, 3), np.float32), np.zeros((2, 4), np.float64)):
        with pytest.raises(ValueError, match=r"float32 \[2, 4\]"):
            f.update_rows(ids, bad, lr=0.5)
    f.feature_dtype = "bfloat16"
    with pytest.raises(ValueError, match="bfloat16"):
        f.update_rows(ids, grads, lr=0.5)
