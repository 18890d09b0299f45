"""The launch geometry of the fused samplers (kivi_amd/csrc/kivi_sample.hip: kivi_sample, kivi_sample_rows, kivi_sample_rows_pen),
restated for the tests from the header and the kernel's comments -- no kernel, no device.

A row of V tokens is drawn by one block of 16 waves.  The host takes the bucket size BS = 64, doubled while BS * 1024 < V, so a row
has nbk = ceil(V / BS) <= 1024 buckets; wave w owns bpw = ceil(nbk / 16) consecutive buckets, the tokens
[min(V, w * bpw * BS), min(V, (w + 1) * bpw * BS)).  The last bucket may be partial, late waves may own nothing.
kivi_sample_rows_pen folds a row's history into one bit per chunk of 64 tokens, read in groups of 512.

VS is the vocabulary list of tests/test_sample_exact_gpu.py and tests/test_sample_edges_gpu.py; tests/test_sample_plan_cpu.py
holds it to the classes it is there for."""
from typing import List, NamedTuple, Tuple

WAVES, WAVE, MAX_BUCKETS, MAX_V = 16, 64, 1024, 1 << 20
CHUNK, GROUP = 64, 512           # the chunk bitmap of the penalised kernel: a bit per 64 tokens, a byte per 512

VS = [1, 2, 63, 64, 65, 1023, 1024, 1025, 4099, 65535, 65536, 65537, 131072, 131073, 151936, 262144, 262145, 1048576]


class Plan(NamedTuple):
    BS: int                              # tokens per bucket
    nbk: int                             # buckets in the row
    bpw: int                             # buckets per wave
    segments: List[Tuple[int, int]]      # [e0, e1) of every wave, empty ones included


def plan(V: int) -> Plan:
    if not 1 <= V <= MAX_V:
        raise ValueError(f"V={V} outside [1, {MAX_V}]")
    BS = WAVE
    while BS * MAX_BUCKETS < V:
        BS <<= 1
    nbk = (V + BS - 1) // BS
    bpw = (nbk + WAVES - 1) // WAVES
    seg = [(min(V, w * bpw * BS), min(V, (w + 1) * bpw * BS)) for w in range(WAVES)]
    return Plan(BS, nbk, bpw, seg)


def last_bucket(V: int) -> Tuple[int, int]:
    """[e0, V) of the row's last bucket (partial when V % BS != 0)."""
    p = plan(V)
    return (p.nbk - 1) * p.BS, V


def boundaries(V: int) -> List[int]:
    """b * BS of the first bucket boundary, a middle one and the last one (fewer when the row has fewer; none for one bucket)."""
    p = plan(V)
    return sorted({b * p.BS for b in (1, p.nbk // 2, p.nbk - 1) if 1 <= b < p.nbk})


def classes(V: int) -> set:
    """The names of the classes of tests/test_sample_plan_cpu.py that V belongs to."""
    p = plan(V)
    out = {f"BS={p.BS}"}
    if V < WAVE:
        out.add("V<64")
    if V % WAVE:
        out.add("V%64")
    if V % p.BS and p.nbk > 1:
        out.add("partial last bucket of several")
    if p.nbk == MAX_BUCKETS:
        out.add("nbk=1024")
    if any(e0 == e1 for e0, e1 in p.segments):
        out.add("empty wave")
    if any(0 < e1 - e0 < p.BS for e0, e1 in p.segments):
        out.add("wave of one partial bucket")
    if p.nbk % WAVES:
        out.add("nbk%16")
    if V % 8:
        out.add("V%8")
    if V % GROUP:
        out.add("V%512")
    return out
