"""Inputs of the per-replicate EM histogram tests (tests/test_bootstrap_em_cpu.py checks what is said here without a
GPU, tests/test_gpu_bootstrap_em.py runs them): 70 closely related variants of one 1,500-bp genome, so that most
passing windows lie in several groups. At k = 21: 20,438 multi-group windows in 3,937 intervals and 603 merged rows
with up to 70 entries, one row holding 7,270 windows. (read_report_inputs.many_ref() has no multi-group window at all.)
The base input of the bootstrap tests (read_report_inputs.base_ref / base_reads: 3 groups) is the other one."""
from __future__ import annotations

from functools import lru_cache

import bootstrap_em_model as bem
import em_reference as er
import read_report_inputs as ri
from speq_amd import synth

CUTOFF = ri.CUTOFF
K = 21
G70 = 70


@lru_cache(maxsize=None)
def ref70():
    return synth.make_reference(G70, 1, 1500)


@lru_cache(maxsize=None)
def reads70():
    rd = synth.make_reads(ref70(), 400, read_len=100, n_rate=0.002, lowq_rate=0.01)
    return rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets


@lru_cache(maxsize=None)
def index70(k: int = K) -> dict:
    ref = ref70()
    return er.build_index(ref.records, ref.groups, G70, k)


@lru_cache(maxsize=None)
def multi70(paired: bool = False) -> bem.MultiUnits:
    return bem.multi_units(index70(), G70, K, *reads70(), CUTOFF, paired)


@lru_cache(maxsize=None)
def base_index(k: int) -> dict:
    ref = ri.base_ref()
    return er.build_index(ref.records, ref.groups, 3, k)


@lru_cache(maxsize=None)
def base_multi(k: int, paired: bool) -> bem.MultiUnits:
    return bem.multi_units(base_index(k), 3, k, *ri.base_reads(k), CUTOFF, paired)
