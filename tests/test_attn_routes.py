"""Which kernel instantiation every attention-forward problem of tests/attn_route_cases.py takes (i2v_attention_route: host arithmetic, no
GPU), that every instantiation of the launch table (i2v_attn_kernel_exists) is the route of at least one case in an environment that
reaches it, that the production shapes keep their routes, that the table holds the edges the kernels have, and that the checker the GPU
test uses (tests/attn_bounds.py) has teeth: on every case a torch emulation of the kernels' arithmetic passes checks (a) and (b) and
the fused-lse bound, plain fp32 SDPA passes check (b), and each of nine slightly wrong evaluations misses."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import attn_bounds as B
from tests import attn_route_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import i2v_adapter_unofficial_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return pkg._lib


def test_abi_version_35_exports_the_route_queries(lib):
    src = open(os.path.join(ROOT, "include", "i2v_hip.h")).read()
    assert int(re.search(r"#define I2V_ABI_VERSION (\d+)", src).group(1)) == lib.ABI_VERSION >= 35
    h = lib.load()
    assert h.i2v_abi_version() == lib.ABI_VERSION
    for sym in ("i2v_attention_route", "i2v_attention_last_route", "i2v_attn_kernel_exists"):
        assert hasattr(h, sym) and sym in lib.SIGNATURES and re.search(rf"\b{sym}\(", src), sym
    assert tuple(n for n, _ in lib.AttnRoute._fields_) == G.ROUTE_FIELDS
    r = lib.AttnRoute()
    assert h.i2v_attention_route(2, 1, 8, 40, 64, 64, None) == -1 and h.i2v_attn_kernel_exists(None) == 0
    # the query refuses what the launch refuses, with the launch's words
    assert h.i2v_attention_route(2, 1, 8, 168, 64, 64, C.byref(r)) == -1 and b"head_dim (168)" in h.i2v_last_error()
    assert h.i2v_attention_route(3, 2, 8, 40, 64, 64, C.byref(r)) == -1 and b"multiple of kv_group" in h.i2v_last_error()
    assert h.i2v_attention_route(2, 1, 8, 40, 0, 64, C.byref(r)) == -1 and h.i2v_attention_route(2, 1, 70000, 40, 64, 64, C.byref(r)) == -1
    p = lib.AttnParams()
    p.q = p.k = p.vt = p.o = 0x7F0000000000
    p.batch_q, p.kv_group, p.heads, p.head_dim, p.lq, p.lk = 2, 1, 8, 168, 64, 64
    assert h.i2v_attention_f16(C.byref(p), None) == -1 and b"i2v_attention_f16: head_dim (168)" in h.i2v_last_error()
    # before this thread's first launch the last route is an error, not stale data; after one it names a kernel of the table
    assert h.i2v_attention_last_route(None) == -1
    if h.i2v_attention_last_route(C.byref(r)) == -1:
        assert b"no i2v_attention_f16 yet" in h.i2v_last_error()
    else:
        assert h.i2v_attn_kernel_exists(C.byref(r)) == 1
    import i2v_adapter_unofficial_amd as pkg
    assert pkg.kernels.attn_route(2, 1, 8, 40, 4096, 77) == G.Rt(64, 48, 1, 2, 96, 0, 1, (32, 8, 2), 1)


def existing_instantiations(lib):
    """the whole space of template arguments (and what lies just outside it), asked through the existence query"""
    h, found = lib.load(), set()
    sizes = (0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 192)
    for dqk, dpv, spare, qt, kvt, walk in itertools.product(sizes, sizes, (-1, 0, 1, 2), (0, 1, 2, 3, 4), (0, 32, 64, 96, 128, 192, 256), (-1, 0, 1, 2)):
        r = lib.AttnRoute(dqk=dqk, dpv=dpv, spare=spare, qt=qt, kvt=kvt, walk=walk, qbw=1, grid_x=1, grid_y=1, grid_z=1)
        if h.i2v_attn_kernel_exists(C.byref(r)):
            found.add((dqk, dpv, spare, qt, kvt, walk))
    return found


def expected_instantiations():
    kv = lambda dqk: (64,) + ((96,) if dqk == 64 else ()) + ((128,) if dqk <= 64 else ())
    return {(dqk, dpv, spare, qt, kvt, walk) for dqk, dpv in G.CLASSES for kvt in kv(dqk) for spare in (0, 1) for qt in (1, 2) for walk in (0, 1)}


def env_reaches(env_name, key):
    """can a problem take this instantiation under this environment (the rules of attn_plan, read off the template arguments)"""
    dqk, dpv, spare, qt, kvt, walk = key
    if env_name == "default":
        return kvt != 128 and not (dqk == 128 and qt == 2)
    if env_name == "walk0":
        return kvt != 128 and not (dqk == 128 and qt == 2) and not walk
    return qt == int(env_name[-1]) and kvt == (128 if dqk <= 64 else 64)


@pytest.mark.parametrize("env_name", list(G.ENVS))
def test_every_case_takes_its_expected_route(lib, env_name):
    """asked in a child that carries the environment's switches (they are read once per process); the child loads the library and calls
    host queries only"""
    env = {k: v for k, v in os.environ.items() if k not in G.SWITCHES}
    env.update(dict(G.ENVS[env_name]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_route_cases.py"), "--routes", env_name], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    cases = G.cases_of(env_name)
    assert len(cases) >= 2 and sorted(got) == sorted(c["name"] for c in cases)
    bad = [f"{c['name']}: {got[c['name']]}, expected {c['route']}" for c in cases if got[c["name"]] != c["route"]]
    assert not bad, f"{len(bad)} of {len(cases)} cases take another kernel than the table says:\n" + "\n".join(bad)


def test_every_instantiation_has_a_case_in_an_environment_that_reaches_it(lib):
    exist = existing_instantiations(lib)
    expected = expected_instantiations()
    assert len(expected) == 112 and exist == expected, sorted(exist ^ expected)
    covered = {G.key_of(c["route"]) for c in G.CASES}
    assert covered <= exist, f"the table expects kernels that do not exist: {sorted(covered - exist)}"
    assert covered == exist, f"{len(exist - covered)} instantiations are no case's route:\n" + "\n".join(map(str, sorted(exist - covered)))
    for c in G.CASES:
        name = next(n for n, e in G.ENVS.items() if e == c["env"])
        assert env_reaches(name, G.key_of(c["route"])), c["name"]
    default = {G.key_of(c["route"]) for c in G.cases_of("default")}
    assert default == {k for k in exist if env_reaches("default", k)} and len(default) == 76
    for name in ("kvt128-qt1", "kvt128-qt2"):
        here = {G.key_of(c["route"]) for c in G.cases_of(name)}
        assert here >= {k for k in exist - default if env_reaches(name, k)}, name
    assert len(exist - default) == 36


def test_the_table_covers_the_edges_the_kernels_have():
    every = G.CASES
    d = G.cases_of("default")
    R = lambda c: c["route"]
    nt = lambda c: -(-c["lk"] // R(c)["kvt"])
    nqb = lambda c: -(-c["lq"] // (64 * R(c)["qt"]))
    one = [c for c in d if not R(c)["walk"]]
    walk = [c for c in d if R(c)["walk"]]
    # ---- sizes: Q within about 2048 x 128 rows x head_dim (the two qbw = 8 problems need 8192 blocks: they use head_dim 8)
    for c in every:
        rows = c["bq"] * c["heads"] * c["lq"]
        assert rows <= 2048 * 128 * 1.05 or (R(c)["qbw"] == 8 or "qbw8" in c["name"]) and c["d"] == 8 and rows <= 2048 * 128 * 4, c["name"]
        if R(c)["walk"] and R(c)["dqk"] >= 96:
            assert nqb(c) in (2, 3), c["name"]
    # ---- key lengths
    assert any(c["lk"] == 1 for c in one) and any(c["lk"] == 1 for c in walk)
    assert {c["lk"] % R(c)["kvt"] for c in one if nt(c) >= 2} >= {1, 7, 8, 9, 63, 0}
    k128 = [c for c in G.cases_of("kvt128-qt1") + G.cases_of("kvt128-qt2") if R(c)["kvt"] == 128]
    assert {c["lk"] % 128 for c in k128 if nt(c) >= 2} >= {1, 7, 8, 9, 127, 0} and {min(nt(c), 5) for c in k128} >= {1, 2, 3, 5}
    assert {min(nt(c), 5) for c in one} >= {1, 2, 3, 5} and {nt(c) % 2 for c in one if nt(c) >= 5} == {0, 1}
    for w in (0, 1):
        assert {c["lk"] for c in d if R(c)["kvt"] == 96 and R(c)["walk"] == w} >= {65, 77, 80, 96}
    assert any(R(c)["dqk"] == 64 and c["lk"] == 64 and R(c)["kvt"] == 64 for c in d) and any(R(c)["dqk"] == 64 and c["lk"] == 65 and R(c)["kvt"] == 96 for c in d)
    assert any(R(c)["dqk"] == 96 and c["lk"] == 77 and R(c)["kvt"] == 64 and nt(c) == 2 for c in d)
    # ---- query lengths
    assert {c["lq"] for c in one} >= {1, 15, 16, 17, 127, 128}
    by = {c["name"]: c for c in every}
    assert R(by["one-c48-q127"])["qt"] == 1 and R(by["one-c48-q128"])["qt"] == 2
    for group in (one, walk):
        assert any(c["lq"] % (64 * R(c)["qt"]) == 1 and nqb(c) >= 2 for c in group)                       # a last block with one row
        assert any(0 < c["lq"] % (64 * R(c)["qt"]) <= 32 * R(c)["qt"] for c in group)                     # ... whose waves 2, 3 have none
    # ---- the walk
    assert {R(c)["qbw"] for c in walk} >= {2, 3, 8}
    assert any(nqb(c) % R(c)["qbw"] for c in walk) and any(nqb(c) == R(c)["qbw"] for c in walk)
    wgs = lambda c: nqb(c) * c["heads"] * c["bq"]
    assert any(wgs(c) == 2047 and not R(c)["walk"] and c["lk"] <= R(c)["kvt"] for c in d) and any(wgs(c) == 2048 and R(c)["walk"] for c in d)
    # ---- the three mappings, for both WALK values, two head-dim classes each, odd head counts, batch_q no multiple of 8; poisoned
    for w in (0, 1):
        for mode in (0, 1, 2):
            cs = [c for c in d if R(c)["walk"] == w and R(c)["remap"] == mode]
            assert len({R(c)["dpv"] for c in cs}) >= 2, (w, mode)
            assert any(c["heads"] in (3, 5, 6, 10) for c in cs) and any(c["bq"] % 8 for c in cs), (w, mode)
    assert all(c["o"] != "own" for c in every if R(c)["remap"] != 0)
    # ---- grouping
    assert {1, 2} <= {c["grp"] for c in d} and any(c["grp"] == c["bq"] > 2 for c in d) and any(c["bq"] % 4 for c in d)
    for group in (one, walk):
        assert any(c["grp"] == 2 and c["bq"] >= 4 for c in group) and any(c["grp"] == c["bq"] > 1 for c in group)
    # ---- head dims: every SPARE size and every full size
    assert {c["d"] for c in d} >= {8, 24, 40, 56, 72, 88, 104, 120, 136, 152, 16, 32, 48, 64, 80, 96, 128, 160}
    # ---- layouts
    assert {c["qk"] for c in d} == set(G.QK) and {c["o"] for c in one} == set(G.OUTPUTS) == {c["o"] for c in walk}
    wide_vt = [c for c in d if c["vt_ld"] > G.pad8(c["lk"])]
    assert any(c["lk"] % R(c)["kvt"] == 0 for c in wide_vt) and any(c["lk"] % R(c)["kvt"] for c in wide_vt) and any(R(c)["walk"] for c in wide_vt)
    # ---- forms: accumulate and the fused lse for every SPARE x QT x WALK
    for form in ("acc", "lse"):
        have = {(R(c)["spare"], R(c)["qt"], R(c)["walk"]) for c in every if c["form"] == form}
        assert have == set(itertools.product((0, 1), (1, 2), (0, 1))), form
    # ---- input families
    for group in (one, walk):
        assert {c["inputs"] for c in group} >= {"unit", "large"}
    for fam in ("spike", "creep"):
        assert {(R(c)["spare"], R(c)["qt"]) for c in one if c["inputs"] == fam} == set(itertools.product((0, 1), (1, 2))), fam
    slots = set()
    for c in every:
        if c["inputs"] == "spike":
            keys = B.spike_keys(c["lk"], R(c)["kvt"])
            assert min(keys) >= R(c)["kvt"] and c["lk"] - 1 in keys and (c["lk"] - 1) // R(c)["kvt"] * R(c)["kvt"] in keys
            used = {keys[p % len(keys)] for p in range(c["bq"] // c["grp"] * c["heads"])}
            slots |= {B.lane_slot(k, R(c)["kvt"]) for k in used}
    assert slots == set(itertools.product(range(4), range(2)))
    # ---- I2V_ATTN_WALK=0: walk-sized problems on the one-trip kernels
    off = G.cases_of("walk0")
    assert 2 <= len(off) <= 3 and all(wgs(c) >= 2048 and c["lk"] <= R(c)["kvt"] and not R(c)["walk"] and R(c)["qbw"] == 1 for c in off)


# the attention launches of the benchmark's configuration (16 frames of 512 x 512: latents 64 x 64, batch 2 for CFG, 8 heads; K1 the
# cross-frame adapter attention with kv_group = frames, K2 spatial self-attention, K3 text (77 tokens) and image-prompt (4 | 16 tokens)
# cross-attention) at each UNet level -> the route at the commit before the route query
PRODUCTION = [
    ("K1 64^2 d40", (32, 16, 8, 40, 4096, 4096), G.Rt(64, 48, 1, 2, 64, 0, 1, (32, 8, 32), 2)),
    ("K2 64^2 d40", (32, 1, 8, 40, 4096, 4096), G.Rt(64, 48, 1, 2, 64, 0, 1, (32, 8, 32), 2)),
    ("K3 64^2 d40 text", (32, 1, 8, 40, 4096, 77), G.Rt(64, 48, 1, 2, 96, 1, 8, (4, 8, 32), 1)),
    ("K3 64^2 d40 ip4", (32, 1, 8, 40, 4096, 4), G.Rt(64, 48, 1, 2, 64, 1, 8, (4, 8, 32), 1)),
    ("K3 64^2 d40 ip16", (32, 1, 8, 40, 4096, 16), G.Rt(64, 48, 1, 2, 64, 1, 8, (4, 8, 32), 1)),
    ("K1 32^2 d80", (32, 16, 8, 80, 1024, 1024), G.Rt(96, 80, 0, 2, 64, 0, 1, (8, 8, 32), 2)),
    ("K2 32^2 d80", (32, 1, 8, 80, 1024, 1024), G.Rt(96, 80, 0, 2, 64, 0, 1, (8, 8, 32), 2)),
    ("K3 32^2 d80 text", (32, 1, 8, 80, 1024, 77), G.Rt(96, 80, 0, 2, 64, 0, 1, (8, 8, 32), 1)),
    ("K3 32^2 d80 ip4", (32, 1, 8, 80, 1024, 4), G.Rt(96, 80, 0, 2, 64, 1, 2, (4, 8, 32), 1)),
    ("K3 32^2 d80 ip16", (32, 1, 8, 80, 1024, 16), G.Rt(96, 80, 0, 2, 64, 1, 2, (4, 8, 32), 1)),
    ("K1 16^2 d160", (32, 16, 8, 160, 256, 256), G.Rt(160, 160, 0, 2, 64, 0, 1, (2, 8, 32), 2)),
    ("K2 16^2 d160", (32, 1, 8, 160, 256, 256), G.Rt(160, 160, 0, 2, 64, 0, 1, (2, 8, 32), 2)),
    ("K3 16^2 d160 text", (32, 1, 8, 160, 256, 77), G.Rt(160, 160, 0, 2, 64, 0, 1, (2, 8, 32), 1)),
    ("K3 16^2 d160 ip4", (32, 1, 8, 160, 256, 4), G.Rt(160, 160, 0, 2, 64, 0, 1, (2, 8, 32), 1)),
    ("K3 16^2 d160 ip16", (32, 1, 8, 160, 256, 16), G.Rt(160, 160, 0, 2, 64, 0, 1, (2, 8, 32), 1)),
    ("K1 8^2 d160", (32, 16, 8, 160, 64, 64), G.Rt(160, 160, 0, 1, 64, 0, 1, (1, 8, 32), 1)),
    ("K2 8^2 d160", (32, 1, 8, 160, 64, 64), G.Rt(160, 160, 0, 1, 64, 0, 1, (1, 8, 32), 1)),
    ("K3 8^2 d160 text", (32, 1, 8, 160, 64, 77), G.Rt(160, 160, 0, 1, 64, 0, 1, (1, 8, 32), 1)),
    ("K3 8^2 d160 ip4", (32, 1, 8, 160, 64, 4), G.Rt(160, 160, 0, 1, 64, 0, 1, (1, 8, 32), 1)),
    ("K3 8^2 d160 ip16", (32, 1, 8, 160, 64, 16), G.Rt(160, 160, 0, 1, 64, 0, 1, (1, 8, 32), 1)),
]


def test_production_shapes_keep_their_routes(lib):
    import i2v_adapter_unofficial_amd as pkg
    for what, sizes, route in PRODUCTION:
        assert pkg.kernels.attn_route(*sizes) == route, what


# ------------------------------------------------------------------------------------------------------------------- the checker
MUTANTS = ("the last key dropped", "key slot lk admitted with logit 0", "P rounded through bf16", "the result rounded through bf16",
           "scale off by 2^-10", "O rescaled but not l at one move", "head h reads head h + 1's V", "K / V of batch bq, not bq / kv_group",
           "two query blocks swapped")
KW = dict(zip(MUTANTS, (dict(drop_last=True), dict(extra_slot=True), dict(p_bf16=True), dict(out_bf16=True), dict(scale_off=True),
                        dict(l_not_rescaled=True), dict(next_head_v=True), dict(wrong_group=True), dict(swap_blocks=True))))


def mutants(c):
    """the mutants that apply to a case, BY ITS STRUCTURE ALONE (not by where the checker is expected to win):
    - a dropped key, a rounding of P and a scale error need two keys (a single key's P is 1.0 at any scale and in any format)
    - the admitted slot (a zero K row, logit 0, V = 0) exists where lk is no multiple of the key tile
    - l can miss a rescale only in a kernel that keeps l apart (not SPARE) and that has a second key tile
    - the next head's V needs two heads, the wrong K / V batch kv_group > 1 and more than one K / V batch, swapped query blocks two
      blocks and two keys (with one key every row of a (batch, head) is v_0)
    What applies and is still accepted is listed in EXEMPT with its reason."""
    r = c["route"]
    m = [MUTANTS[3]]
    if c["lk"] >= 2:
        m += [MUTANTS[0], MUTANTS[2], MUTANTS[4]]
    if c["lk"] % r["kvt"]:
        m.append(MUTANTS[1])
    if not r["spare"] and c["lk"] > r["kvt"]:
        m.append(MUTANTS[5])
    if c["heads"] > 1:
        m.append(MUTANTS[6])
    if c["grp"] > 1 and c["bq"] // c["grp"] > 1:
        m.append(MUTANTS[7])
    if c["lq"] > 64 * r["qt"] and c["lk"] >= 2:
        m.append(MUTANTS[8])
    return m


# (case, mutant) pairs that apply by structure and that the checks still accept, each group with its reason.  At most a tenth of all
# pairs (test_every_mutant_applies_in_every_form_and_few_pairs_are_exempt counts them).
EXEMPT = {}


def _exempt(mutant, reason, *names):
    for n in names:
        EXEMPT[n, mutant] = reason


# ---- O rescaled but not l at one move, `heavy` family
_exempt(MUTANTS[5], "no row of this case moves its reference after the first tile: the mutant changes nothing",
         "one-c96-qt1-q17-k73")
# ---- O rescaled but not l at one move, `large` family
_exempt(MUTANTS[5], "no row of this case moves its reference after the first tile: the mutant changes nothing",
         "qt1-one-c16-qt1-q15-k129")
# ---- P rounded through bf16, `heavy` family
_exempt(MUTANTS[2], "a SPARE kernel sums l from the same rounded P, so most of the rounding cancels in the ratio; what is left stays within 2^-10 (W + 2 |ref|)",
         "one-c64s-qt1-q33-k321", "one-c128s-qt1-q127-k128", "qt2-one-c16s-qt2-q128-k257")
# ---- P rounded through bf16, `large` family
_exempt(MUTANTS[2], "most rows are one-hot (P = 1 exactly in either format); on the others the derived fp32 logit term of logits near 100 exceeds 2^-8",
         "one-c16s-qt2-q128-k65", "one-c64s-qt2-q193-k13", "one-c128-qt1-q65-k64", "one-c48s-qt2-q130-k191", "one-c80s-qt2-q128-k319",
         "one96-c48s-qt2-q128-k77", "one96-c64s-qt2-q128-k77", "w96-walk-c64s-qt1-q100-k65", "walk-c64s-qt2-q129-k57",
         "walk-c96-qt1-q100-k40", "walk-c80-qt2-q129-k63", "one-c160-large-5-tiles", "qt1-one-c16-qt1-q15-k129",
         "w96-walk-c64-qt2-q129-k96", "walk-c128-qt1-q100-k64", "qt2-walk-c128s-q129-k64", "walk-c160-qt1-q100-k9", "walk0-c80-h6")
# ---- P rounded through bf16, `spike` family
_exempt(MUTANTS[2], "a row the spiked key wins is one-hot and exact in either format; on the others more than sixty keys share the weight and the roundings average out",
         "one-c16-qt1-q15-k71", "one-c48-qt1-q65-k192", "one-c32s-qt2-q257-k127", "one-c96-qt2-q145-k127", "one-c160s-qt1-q33-k129",
         "one-c160-qt2-q256-k263", "one-remap2-h10", "one-remap0-h5", "qt1-one-c32s-qt1-q16-k135", "qt1-one-c32-qt1-q17-k136",
         "qt1-one-c48-qt1-q65-k255", "qt2-one-c32s-qt2-q257-k384", "qt2-one-c128s-q128-k129")
# ---- key slot lk admitted with logit 0, `creep` family
_exempt(MUTANTS[1], "the two raised keys lie 8 and 10 log2 units above the slot's logit 0: its share of the weight is below 2^-10",
         "one-c48-qt2-q256-k263", "one-c160s-qt2-q130-k191", "one-c48-creep-6-tiles", "one-c64-creep-rn", "one-c48s-creep-qt1",
         "one-remap2-h6", "qt2-one-c128s-q257-k200")
# ---- key slot lk admitted with logit 0, `heavy` family
_exempt(MUTANTS[1], "the slot's logit 0 lies some ten log2 units below the heavy keys of the row: its share of the weight is below the fp16 roundings",
         "one-c32s-qt1-q16-k73", "one-c96s-qt1-q16-k71", "one-c64s-qt1-q33-k321", "one-c64-qt1-q64-k63", "one-c96-qt1-q17-k73",
         "one-c80s-qt1-q1-k137", "one-c48s-qt1-q127-k129", "one-c16s-qt1-q1-k1", "one96-c64s-qt1-q17-k65", "one96-c64-qt1-q127-k80",
         "one-c48-k65", "one-c96-k77", "one-c48-q127", "one-c48-q128", "qt1-one-c48s-qt1-q127-k137", "qt1-walk-c32-qt1-q127-k127",
         "one-remap1-h5-b12", "qt1-walk-c48-qt1-q65-k121", "qt2-one-c16s-qt2-q128-k257", "qt2-one-c48s-qt2-q130-k641",
         "qt2-one-c64s-qt2-q193-k127", "qt2-walk-c32-qt2-q129-k127", "qt2-walk-c48-qt2-q129-k121", "one96-c48s-qt1-q17-k65")
# ---- key slot lk admitted with logit 0, `large` family
_exempt(MUTANTS[1], "nearly every row's maximum lies tens of log2 units above the slot's logit 0: its weight vanishes",
         "one-c16s-qt2-q128-k65", "one-c48s-qt2-q130-k191", "one-c80s-qt2-q128-k319", "one96-c48s-qt2-q128-k77",
         "one96-c64s-qt2-q128-k77", "w96-walk-c48s-qt2-q129-k77", "w96-walk-c64s-qt1-q100-k65", "walk-c64s-qt2-q129-k57",
         "walk-c96-qt1-q100-k40", "walk-c80-qt2-q129-k63", "one-c160-large-5-tiles", "qt1-one-c16-qt1-q15-k129", "walk-qbw3",
         "qt2-one-c16-qt2-q129-k383")
# ---- key slot lk admitted with logit 0, `spike` family
_exempt(MUTANTS[1], "on the rows the spiked key wins the slot has no weight; on the others more than a hundred keys share it and |ref| is a small part of W",
         "one-c160-qt2-q256-k263", "qt1-one-c48-qt1-q65-k255")
# ---- scale off by 2^-10, `creep` family
_exempt(MUTANTS[4], "the logits are below 10 log2 units: the shift of 2^-10 |t| moves the 4 : 1 split of the two raised keys by less than the fp16 roundings",
         "one-c160s-qt2-q130-k191", "one-c64-creep-rn", "one-c48s-creep-qt1", "one-remap2-h6")
# ---- scale off by 2^-10, `heavy` family
_exempt(MUTANTS[4], "the logits of this case stay below 10 log2 units: a shift of 2^-10 |t| is within the fp16 roundings",
         "one-c128s-qt1-q127-k128")
# ---- scale off by 2^-10, `spike` family
_exempt(MUTANTS[4], "the winning rows are one-hot at any scale; the others have logits of a few log2 units, whose shift is within the fp16 roundings",
         "one-c16-qt1-q15-k71")
# ---- scale off by 2^-10, `unit` family
_exempt(MUTANTS[4], "logits of a few log2 units: a shift of 2^-10 |t| is within the fp16 roundings",
         "one-c48-k64")


def judge(c):
    """(messages of what should pass and does not, the accepted mutants, error / bound of the emulation per check, and of the mutants)"""
    t, ev = B.reference(c)
    out, lse = B.emulate(c, t)
    wrong = [B.check(c, out)]
    if c["form"] == "lse":
        wrong.append(B.check_lse(c, lse))
    wrong.append(B.check(c, B.emulate(c, t, plain=True)[0], which=("b",)))
    r = B.ratios(c, out, lse if c["form"] == "lse" else None)
    accepted, mr = [], {}
    for name in mutants(c):
        mo, ml = B.emulate(c, t, **KW[name])
        ml = ml if c["form"] == "lse" else None
        msg = B.check(c, mo) or (B.check_lse(c, ml) if ml is not None else None)
        mr[name] = max(B.ratios(c, mo, ml).values()) if bool(torch.isfinite(mo.float()).all()) else float("inf")
        if msg is None:
            accepted.append(name)
    return [w for w in wrong if w is not None], accepted, r, mr


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c["name"])
def test_the_checker_has_teeth(c):
    """the bounds are conditions on any evaluation in fp32 with P and the result rounded to fp16, so the emulation of the kernels'
    arithmetic must pass (a), (b) and the lse bound, and plain fp32 SDPA (b); and they are tight enough that each slightly wrong
    evaluation misses one of them"""
    wrong, accepted, r, mr = judge(c)
    print(f"{c['name']}: error / bound of the emulation {r}; of the mutants {mr}")
    assert not wrong, "a correct evaluation misses the bound: it is derived wrongly\n" + "\n".join(wrong)
    unexplained = [m for m in accepted if (c["name"], m) not in EXEMPT]
    assert not unexplained, f"the checker accepts the mutants {unexplained}"
    stale = [m for (n, m) in EXEMPT if n == c["name"] and m not in accepted]
    assert not stale, f"exempt, but the checker does reject {stale}"


def test_every_mutant_applies_in_every_form_and_few_pairs_are_exempt():
    pairs = 0
    for spare, walk in itertools.product((0, 1), (0, 1)):
        group = [c for c in G.CASES if c["route"]["spare"] == spare and c["route"]["walk"] == walk]
        names = {m for c in group for m in mutants(c) if (c["name"], m) not in EXEMPT}          # applied AND rejected somewhere
        want = set(MUTANTS) - ({MUTANTS[5]} if spare or walk else set())      # (l kept apart and a second key tile: not SPARE, not WALK)
        assert names >= want, (spare, walk, sorted(want - names))
        pairs += sum(len(mutants(c)) for c in group)
    assert all(m in mutants(next(c for c in G.CASES if c["name"] == n)) for n, m in EXEMPT)
    assert pairs >= 900 and len(EXEMPT) * 10 <= pairs, (len(EXEMPT), pairs)
    # the multi-tile loop and the deferred maximum are shown to reject the roundings too, not only single-tile cases
    for m in (MUTANTS[2], MUTANTS[3], MUTANTS[4]):
        assert sum(1 for c in G.CASES if c["lk"] > 2 * c["route"]["kvt"] and m in mutants(c) and (c["name"], m) not in EXEMPT) >= 10, m
