"""CPU: the vocabulary list of the sampler edge tests (tests/sample_plan.py: VS) covers every class of launch geometry it is there
for, and plan() is a consistent restatement of the geometry of kivi_amd/csrc/kivi_sample.hip.  No device, no kernel."""
import os
import re

import pytest

from sample_plan import MAX_BUCKETS, MAX_V, VS, WAVES, boundaries, classes, last_bucket, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["BS=64", "BS=128", "BS=256", "BS=512", "BS=1024", "V<64", "V%64", "partial last bucket of several", "nbk=1024",
            "empty wave", "wave of one partial bucket", "nbk%16", "V%8", "V%512"]


def test_vocabulary_list_covers_every_class():
    have = {}
    for V in VS:
        for c in classes(V):
            have.setdefault(c, []).append(V)
    missing = [c for c in REQUIRED if c not in have]
    assert not missing, missing
    assert VS == sorted(set(VS)) and VS[0] == 1 and VS[-1] == MAX_V
    # both sides of every step of the bucket size that the list claims to straddle, and of the step from 16 to 17 buckets
    for lo in (1024, 65536, 131072, 262144):
        assert lo in VS and lo + 1 in VS, lo
        assert plan(lo).BS != plan(lo + 1).BS or plan(lo).bpw != plan(lo + 1).bpw, lo
    assert (plan(1024).bpw, plan(1025).bpw) == (1, 2) and plan(1025).segments[8] == (1024, 1025)
    assert all(e0 == e1 for e0, e1 in plan(1025).segments[9:])
    assert (plan(65536).BS, plan(65536).nbk, plan(65537).BS, plan(65537).nbk) == (64, 1024, 128, 513)
    assert (plan(131072).BS, plan(131073).BS, plan(262145).BS, plan(MAX_V).BS) == (128, 256, 512, 1024)


@pytest.mark.parametrize("V", VS + [3, 100, 511, 512, 513, 2047, 32000, 128256, 524288, 524289, MAX_V - 1])
def test_plan_is_consistent(V):
    p = plan(V)
    assert p.BS >= 64 and p.BS & (p.BS - 1) == 0 and p.BS * MAX_BUCKETS >= V
    assert p.BS == 64 or (p.BS // 2) * MAX_BUCKETS < V                       # the smallest such power of two
    assert 1 <= p.nbk <= MAX_BUCKETS and (p.nbk - 1) * p.BS < V <= p.nbk * p.BS
    assert p.bpw * WAVES >= p.nbk > (p.bpw - 1) * WAVES
    assert len(p.segments) == WAVES and p.segments[0][0] == 0 and p.segments[-1][1] == V
    for w, (e0, e1) in enumerate(p.segments):
        assert 0 <= e0 <= e1 <= V
        assert (e0 % p.BS == 0 or e0 == V) and (e1 % p.BS == 0 or e1 == V)
        assert e1 - e0 <= p.bpw * p.BS
        if w:
            assert p.segments[w - 1][1] == e0                                # the segments tile [0, V) in order
    e0, e1 = last_bucket(V)
    assert e1 == V and 0 < e1 - e0 <= p.BS and e0 % p.BS == 0
    for b in boundaries(V):
        assert 0 < b < V and b % p.BS == 0
    assert (not boundaries(V)) == (p.nbk == 1)
    with pytest.raises(ValueError):
        plan(0)
    with pytest.raises(ValueError):
        plan(MAX_V + 1)


def test_the_kernel_source_states_the_same_geometry():
    """Every entry sizes the bucket with the one loop of bucket_size() -- kivi_sample itself, the three row entries through their one
    launch function -- and the row body derives buckets and segments as plan() does."""
    src = open(os.path.join(ROOT, "kivi_amd", "csrc", "kivi_sample.hip")).read()
    assert len(re.findall(r"int BS = KIVI_WAVE;[^\n]*\n\s*while \(\(int64_t\)BS \* 1024 < V\) BS <<= 1;", src)) == 1
    assert len(re.findall(r"BS\s*<<=", src)) == 1 and len(re.findall(r"const int BS = bucket_size\(V\);", src)) == 2
    for entry in ("kivi_sample_rows", "kivi_sample_rows_pen", "kivi_sample_rows_con"):
        assert re.search(r'extern "C" int %s\([^{]*\{\s*return launch_rows\("%s",' % (entry, entry), src)
    assert "constexpr int kThreads = 1024;" in src and "constexpr int kWaves = kThreads / KIVI_WAVE;" in src
    assert "const int nbk = (V + BS - 1) / BS, bpw = (nbk + kWaves - 1) / kWaves;" in src
    assert "const int bk0 = min(nbk, wave * bpw), bk1 = min(nbk, (wave + 1) * bpw);" in src
    assert "const int e0 = min(V, bk0 * BS), e1 = min(V, bk1 * BS);" in src
    hdr = open(os.path.join(ROOT, "include", "kivi_hip.h")).read()
    assert re.search(r"#define\s+KIVI_SAMPLE_MAX_V\s+\(?\s*1\s*<<\s*20\s*\)?|#define\s+KIVI_SAMPLE_MAX_V\s+1048576", hdr)
