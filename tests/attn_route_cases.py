"""The cases of tests/test_attn_routes.py (CPU) and tests/test_attn_routes_gpu.py: one table of attention-forward problems
(kernels.attention -> i2v_attention_f16), each with the environment it runs under and THE ROUTE IT IS EXPECTED TO TAKE, written out
literally (`i2v_attn_route`: which of the library's 112 kernel instantiations runs it, with which grid, how many query blocks a
workgroup walks and which workgroup-to-block mapping).  The shapes are the smallest that reach each instantiation, found on the CPU with
the route query and then written down (`python tests/attn_route_cases.py --routes ENV` prints what the library answers today for the
cases of one environment); a threshold that moves makes the CPU test fail here instead of moving a case silently to another kernel.

A case is `case(name, route, env=..., bq, grp, heads, d, lq, lk, vt_ld=None, qk="own", o="own", form="plain", inputs="unit")`:
  bq, grp     batch_q and kv_group: K / V^T have bq / grp batches, query batch b reads K / V^T batch b // grp
  vt_ld       row stride of V^T [bq / grp, C, vt_ld]; None = pad8(lk).  Columns lk .. vt_ld hold NaN.
  qk          "own": q and k are matrices [rows, C] of their own.  "2C" / "3C": q is the column slice [0, C) of one [rows, 2 C] (3 C)
              matrix and k the column slice [C, 2 C) of another (they differ in rows: lq and lk), the rest holds NaN.
  o           "own": a [rows, C] tensor.  "wide": columns [8, 8 + C) of a poisoned [rows + 3, C + 16] buffer (row stride a multiple of
              8).  "odd": columns [4, 4 + C) of a poisoned [rows + 3, C + 12] buffer (row stride = 4 mod 8).
  form        "plain"; "acc": accumulate onto a previous result with acc_scale 0.75; "lse": return_lse="fused"
  inputs      "unit" / "heavy" / "large" / "spike" / "creep": the input family (tests/attn_bounds.py)
The expected route is Rt(dqk, dpv, spare, qt, kvt, walk, qbw, (grid_x, grid_y, grid_z), remap).

The rules the table was found with (csrc/attention.hip, attn_plan): head_dim takes the first class <dqk, dpv> whose dpv holds it, spare =
head_dim < dpv; qt = 2 from lq >= 128 on except in the <128, 128> class; kvt = 96 for dqk = 64 and 64 < lk <= 96, else 64; nqb =
ceil(lq / (64 qt)); a single key tile (lk <= kvt) with nqb heads bq >= 2048 workgroups walks qbw = min(nqb heads bq / 1024, 8, nqb)
blocks per workgroup; grid = (ceil(nqb / qbw), heads, bq); remap 1 if lk <= 128 and grid_x grid_z % 8 == 0, else 2 if grid_y grid_z
% 8 == 0, else 0."""
import ctypes as C
import os
import sys

SWITCHES = ("I2V_ATTN_KVT", "I2V_ATTN_QT", "I2V_ATTN_WALK")
DEFAULT = ()
KVT128_QT1 = (("I2V_ATTN_KVT", "128"), ("I2V_ATTN_QT", "1"))
KVT128_QT2 = (("I2V_ATTN_KVT", "128"), ("I2V_ATTN_QT", "2"))
WALK0 = (("I2V_ATTN_WALK", "0"),)
ENVS = {"default": DEFAULT, "kvt128-qt1": KVT128_QT1, "kvt128-qt2": KVT128_QT2, "walk0": WALK0}

CLASSES = ((32, 16), (32, 32), (64, 48), (64, 64), (96, 80), (96, 96), (128, 128), (160, 160))
FAMILIES = ("unit", "heavy", "large", "spike", "creep")
OUTPUTS = ("own", "wide", "odd")
FORMS = ("plain", "acc", "lse")
QK = ("own", "2C", "3C")
ACC_SCALE = 0.75
ROUTE_FIELDS = ("dqk", "dpv", "spare", "qt", "kvt", "walk", "qbw", "grid_x", "grid_y", "grid_z", "remap")
KEY_FIELDS = ROUTE_FIELDS[:6]          # the template arguments: what names an instantiation


def Rt(dqk, dpv, spare, qt, kvt, walk, qbw, grid, remap):
    return dict(dqk=dqk, dpv=dpv, spare=spare, qt=qt, kvt=kvt, walk=walk, qbw=qbw, grid_x=grid[0], grid_y=grid[1], grid_z=grid[2],
                remap=remap)


def pad8(n):
    return (n + 7) // 8 * 8


def key_of(route):
    return tuple(route[f] for f in KEY_FIELDS)


CASES = []


def case(name, route, env=DEFAULT, *, bq, grp, heads, d, lq, lk, vt_ld=None, qk="own", o="own", form="plain", inputs="unit"):
    assert all(c["name"] != name for c in CASES), name
    assert o in OUTPUTS and inputs in FAMILIES and form in FORMS and qk in QK and bq % grp == 0, name
    CASES.append(dict(name=name, route=route, env=env, bq=bq, grp=grp, heads=heads, d=d, lq=lq, lk=lk,
                      vt_ld=pad8(lk) if vt_ld is None else vt_ld, qk=qk, o=o, form=form, inputs=inputs))


# ============================================================================================ the table
# ---- default environment, 64-key tiles: every class x SPARE x QT, one-trip and walking
case("one-c16s-qt1-q1-k1", Rt(32, 16, 1, 1, 64, 0, 1, (1, 1, 1), 0), bq=1, grp=1, heads=1, d=8, lq=1, lk=1, o='own', form='acc', inputs='heavy')
case("one-c16s-qt2-q128-k65", Rt(32, 16, 1, 2, 64, 0, 1, (1, 2, 3), 0), bq=3, grp=1, heads=2, d=8, lq=128, lk=65, vt_ld=80, o='wide', form='acc', inputs='large')
case("one-c16-qt1-q15-k71", Rt(32, 16, 0, 1, 64, 0, 1, (1, 3, 2), 0), bq=2, grp=2, heads=3, d=16, lq=15, lk=71, qk='2C', o='odd', form='acc', inputs='spike')
case("one-c16-qt2-q129-k72", Rt(32, 16, 0, 2, 64, 0, 1, (2, 5, 3), 0), bq=3, grp=3, heads=5, d=16, lq=129, lk=72, vt_ld=96, o='own', form='acc', inputs='spike')
case("one-c32s-qt1-q16-k73", Rt(32, 32, 1, 1, 64, 0, 1, (1, 6, 4), 2), bq=4, grp=2, heads=6, d=24, lq=16, lk=73, qk='3C', o='wide', form='lse', inputs='heavy')
case("one-c32s-qt2-q257-k127", Rt(32, 32, 1, 2, 64, 0, 1, (3, 3, 8), 1), bq=8, grp=2, heads=3, d=24, lq=257, lk=127, o='odd', form='lse', inputs='spike')
case("one-c32-qt1-q17-k128", Rt(32, 32, 0, 1, 64, 0, 1, (1, 10, 4), 2), bq=4, grp=4, heads=10, d=32, lq=17, lk=128, vt_ld=136, o='wide', form='lse', inputs='heavy')
case("one-c32-qt2-q145-k64", Rt(32, 32, 0, 2, 64, 0, 1, (2, 5, 6), 0), bq=6, grp=1, heads=5, d=32, lq=145, lk=64, qk='2C', o='wide', form='lse', inputs='heavy')
case("one-c48s-qt1-q127-k129", Rt(64, 48, 1, 1, 64, 0, 1, (2, 2, 5), 0), bq=5, grp=5, heads=2, d=40, lq=127, lk=129, vt_ld=160, o='odd', inputs='heavy')
case("one-c48s-qt2-q130-k191", Rt(64, 48, 1, 2, 64, 0, 1, (2, 3, 3), 0), bq=3, grp=1, heads=3, d=40, lq=130, lk=191, qk='3C', o='own', inputs='large')
case("one-c48-qt1-q65-k192", Rt(64, 48, 0, 1, 64, 0, 1, (2, 6, 4), 2), bq=4, grp=1, heads=6, d=48, lq=65, lk=192, o='wide', inputs='spike')
case("one-c48-qt2-q256-k263", Rt(64, 48, 0, 2, 64, 0, 1, (2, 1, 7), 0), bq=7, grp=7, heads=1, d=48, lq=256, lk=263, vt_ld=272, o='odd', inputs='creep')
case("one-c64s-qt1-q33-k321", Rt(64, 64, 1, 1, 64, 0, 1, (1, 1, 1), 0), bq=1, grp=1, heads=1, d=56, lq=33, lk=321, qk='2C', o='own', form='acc', inputs='heavy')
case("one-c64s-qt2-q193-k13", Rt(64, 64, 1, 2, 64, 0, 1, (2, 2, 3), 0), bq=3, grp=1, heads=2, d=56, lq=193, lk=13, vt_ld=40, o='wide', form='acc', inputs='large')
case("one-c64-qt1-q64-k63", Rt(64, 64, 0, 1, 64, 0, 1, (1, 3, 2), 0), bq=2, grp=2, heads=3, d=64, lq=64, lk=63, qk='3C', o='odd', form='acc', inputs='heavy')
case("one-c64-qt2-q385-k9", Rt(64, 64, 0, 2, 64, 0, 1, (4, 5, 3), 0), bq=3, grp=3, heads=5, d=64, lq=385, lk=9, o='own', form='acc', inputs='heavy')
case("one-c80s-qt1-q1-k137", Rt(96, 80, 1, 1, 64, 0, 1, (1, 6, 4), 2), bq=4, grp=2, heads=6, d=72, lq=1, lk=137, vt_ld=152, o='wide', form='lse', inputs='heavy')
case("one-c80s-qt2-q128-k319", Rt(96, 80, 1, 2, 64, 0, 1, (1, 3, 8), 2), bq=8, grp=2, heads=3, d=72, lq=128, lk=319, qk='2C', o='odd', form='lse', inputs='large')
case("one-c80-qt1-q15-k1", Rt(96, 80, 0, 1, 64, 0, 1, (1, 10, 4), 2), bq=4, grp=4, heads=10, d=80, lq=15, lk=1, vt_ld=32, o='wide', form='lse', inputs='large')
case("one-c80-qt2-q129-k65", Rt(96, 80, 0, 2, 64, 0, 1, (2, 5, 6), 0), bq=6, grp=1, heads=5, d=80, lq=129, lk=65, qk='3C', o='wide', form='lse', inputs='spike')
case("one-c96s-qt1-q16-k71", Rt(96, 96, 1, 1, 64, 0, 1, (1, 2, 5), 0), bq=5, grp=5, heads=2, d=88, lq=16, lk=71, o='odd', inputs='heavy')
case("one-c96s-qt2-q257-k72", Rt(96, 96, 1, 2, 64, 0, 1, (3, 3, 3), 0), bq=3, grp=1, heads=3, d=88, lq=257, lk=72, vt_ld=80, o='own', inputs='spike')
case("one-c96-qt1-q17-k73", Rt(96, 96, 0, 1, 64, 0, 1, (1, 6, 4), 2), bq=4, grp=1, heads=6, d=96, lq=17, lk=73, qk='2C', o='wide', inputs='heavy')
case("one-c96-qt2-q145-k127", Rt(96, 96, 0, 2, 64, 0, 1, (2, 1, 7), 0), bq=7, grp=7, heads=1, d=96, lq=145, lk=127, vt_ld=152, o='odd', inputs='spike')
case("one-c128s-qt1-q127-k128", Rt(128, 128, 1, 1, 64, 0, 1, (2, 1, 1), 0), bq=1, grp=1, heads=1, d=104, lq=127, lk=128, qk='3C', o='own', form='acc', inputs='heavy')
case("one-c128-qt1-q65-k64", Rt(128, 128, 0, 1, 64, 0, 1, (2, 2, 3), 0), bq=3, grp=1, heads=2, d=128, lq=65, lk=64, o='wide', form='acc', inputs='large')
case("one-c160s-qt1-q33-k129", Rt(160, 160, 1, 1, 64, 0, 1, (1, 3, 2), 0), bq=2, grp=2, heads=3, d=136, lq=33, lk=129, vt_ld=144, o='odd', form='lse', inputs='spike')
case("one-c160s-qt2-q130-k191", Rt(160, 160, 1, 2, 64, 0, 1, (2, 5, 3), 0), bq=3, grp=3, heads=5, d=152, lq=130, lk=191, qk='2C', o='own', form='acc', inputs='creep')
case("one-c160-qt1-q64-k192", Rt(160, 160, 0, 1, 64, 0, 1, (1, 6, 4), 2), bq=4, grp=2, heads=6, d=160, lq=64, lk=192, vt_ld=216, o='wide', form='lse', inputs='heavy')
case("one-c160-qt2-q256-k263", Rt(160, 160, 0, 2, 64, 0, 1, (2, 3, 8), 2), bq=8, grp=2, heads=3, d=160, lq=256, lk=263, qk='3C', o='odd', form='acc', inputs='spike')
case("walk-c16s-qt1-q127-k1", Rt(32, 16, 1, 1, 64, 1, 2, (1, 8, 128), 1), bq=128, grp=1, heads=8, d=8, lq=127, lk=1, o='wide', form='lse')
case("walk-c16s-qt2-q129-k64", Rt(32, 16, 1, 2, 64, 1, 2, (1, 6, 172), 2), bq=172, grp=2, heads=6, d=8, lq=129, lk=64, o='wide', vt_ld=72, form='lse', inputs='large')
case("walk-c16-qt1-q65-k13", Rt(32, 16, 0, 1, 64, 1, 2, (1, 3, 343), 0), bq=343, grp=343, heads=3, d=16, lq=65, lk=13, o='odd', form='lse', inputs='heavy')
case("walk-c16-qt2-q129-k63", Rt(32, 16, 0, 2, 64, 1, 2, (1, 5, 208), 1), bq=208, grp=2, heads=5, d=16, lq=129, lk=63, o='odd', form='lse', inputs='heavy')
case("walk-c32s-qt1-q100-k9", Rt(32, 32, 1, 1, 64, 1, 2, (1, 10, 108), 2), bq=108, grp=4, heads=10, d=24, lq=100, lk=9, o='wide', form='acc', inputs='large')
case("walk-c32s-qt2-q129-k57", Rt(32, 32, 1, 2, 64, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=24, lq=129, lk=57, o='odd', vt_ld=72, form='acc', inputs='heavy')
case("walk-c32-qt1-q127-k40", Rt(32, 32, 0, 1, 64, 1, 2, (1, 4, 256), 1), bq=256, grp=256, heads=4, d=32, lq=127, lk=40, o='wide', form='acc')
case("walk-c32-qt2-q129-k2", Rt(32, 32, 0, 2, 64, 1, 2, (1, 12, 86), 2), bq=86, grp=2, heads=12, d=32, lq=129, lk=2, o='wide', form='acc', inputs='large')
case("walk-c48s-qt1-q65-k1", Rt(64, 48, 1, 1, 64, 1, 2, (1, 8, 128), 1), bq=128, grp=1, heads=8, d=40, lq=65, lk=1, o='odd', inputs='heavy')
case("walk-c48s-qt2-q129-k64", Rt(64, 48, 1, 2, 64, 1, 2, (1, 6, 172), 2), bq=172, grp=2, heads=6, d=40, lq=129, lk=64, o='odd', vt_ld=72, inputs='heavy')
case("walk-c48-qt1-q100-k13", Rt(64, 48, 0, 1, 64, 1, 2, (1, 3, 343), 0), bq=343, grp=343, heads=3, d=48, lq=100, lk=13, o='wide', inputs='large')
case("walk-c48-qt2-q129-k63", Rt(64, 48, 0, 2, 64, 1, 2, (1, 5, 208), 1), bq=208, grp=2, heads=5, d=48, lq=129, lk=63, o='odd', inputs='heavy')
case("walk-c64s-qt1-q127-k9", Rt(64, 64, 1, 1, 64, 1, 2, (1, 10, 108), 2), bq=108, grp=4, heads=10, d=56, lq=127, lk=9, o='wide', form='lse')
case("walk-c64s-qt2-q129-k57", Rt(64, 64, 1, 2, 64, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=56, lq=129, lk=57, o='wide', vt_ld=72, form='lse', inputs='large')
case("walk-c64-qt1-q65-k40", Rt(64, 64, 0, 1, 64, 1, 2, (1, 4, 256), 1), bq=256, grp=256, heads=4, d=64, lq=65, lk=40, o='odd', form='lse', inputs='heavy')
case("walk-c64-qt2-q129-k2", Rt(64, 64, 0, 2, 64, 1, 2, (1, 12, 86), 2), bq=86, grp=2, heads=12, d=64, lq=129, lk=2, o='odd', form='lse')
case("walk-c80s-qt1-q100-k1", Rt(96, 80, 1, 1, 64, 1, 2, (1, 8, 128), 1), bq=128, grp=1, heads=8, d=72, lq=100, lk=1, o='wide', form='acc', inputs='large')
case("walk-c80s-qt2-q129-k64", Rt(96, 80, 1, 2, 64, 1, 2, (1, 6, 172), 2), bq=172, grp=2, heads=6, d=72, lq=129, lk=64, o='odd', vt_ld=72, form='acc', inputs='heavy')
case("walk-c80-qt1-q127-k13", Rt(96, 80, 0, 1, 64, 1, 2, (1, 3, 343), 0), bq=343, grp=343, heads=3, d=80, lq=127, lk=13, o='own', form='acc')
case("walk-c80-qt2-q129-k63", Rt(96, 80, 0, 2, 64, 1, 2, (1, 5, 208), 1), bq=208, grp=2, heads=5, d=80, lq=129, lk=63, o='wide', form='acc', inputs='large')
case("walk-c96s-qt1-q65-k9", Rt(96, 96, 1, 1, 64, 1, 2, (1, 10, 108), 2), bq=108, grp=4, heads=10, d=88, lq=65, lk=9, o='odd', inputs='heavy')
case("walk-c96s-qt2-q129-k57", Rt(96, 96, 1, 2, 64, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=88, lq=129, lk=57, o='own', vt_ld=72, inputs='heavy')
case("walk-c96-qt1-q100-k40", Rt(96, 96, 0, 1, 64, 1, 2, (1, 4, 256), 1), bq=256, grp=256, heads=4, d=96, lq=100, lk=40, o='wide', inputs='large')
case("walk-c96-qt2-q129-k2", Rt(96, 96, 0, 2, 64, 1, 2, (1, 12, 86), 2), bq=86, grp=2, heads=12, d=96, lq=129, lk=2, o='odd', inputs='heavy')
case("walk-c128s-qt1-q127-k1", Rt(128, 128, 1, 1, 64, 1, 2, (1, 8, 128), 1), bq=128, grp=1, heads=8, d=120, lq=127, lk=1, o='wide', form='lse')
case("walk-c128-qt1-q100-k64", Rt(128, 128, 0, 1, 64, 1, 2, (1, 6, 172), 2), bq=172, grp=2, heads=6, d=128, lq=100, lk=64, o='wide', vt_ld=72, form='lse', inputs='large')
case("walk-c160s-qt1-q65-k13", Rt(160, 160, 1, 1, 64, 1, 2, (1, 3, 343), 0), bq=343, grp=343, heads=3, d=152, lq=65, lk=13, o='odd', form='acc', inputs='heavy')
case("walk-c160s-qt2-q129-k63", Rt(160, 160, 1, 2, 64, 1, 2, (1, 5, 208), 1), bq=208, grp=2, heads=5, d=136, lq=129, lk=63, o='odd', form='lse', inputs='heavy')
case("walk-c160-qt1-q100-k9", Rt(160, 160, 0, 1, 64, 1, 2, (1, 10, 108), 2), bq=108, grp=4, heads=10, d=160, lq=100, lk=9, o='wide', form='acc', inputs='large')
case("walk-c160-qt2-q129-k57", Rt(160, 160, 0, 2, 64, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=160, lq=129, lk=57, o='odd', vt_ld=72, form='lse', inputs='heavy')
# ---- default environment, 96-key tiles (dqk = 64, 64 < lk <= 96): lk = 65, 77, 80, 96
case("one96-c48s-qt1-q17-k65", Rt(64, 48, 1, 1, 96, 0, 1, (1, 3, 3), 0), bq=3, grp=1, heads=3, d=40, lq=17, lk=65, o='own', inputs='heavy')
case("one96-c48s-qt2-q128-k77", Rt(64, 48, 1, 2, 96, 0, 1, (1, 3, 3), 0), bq=3, grp=1, heads=3, d=40, lq=128, lk=77, o='odd', form='acc', vt_ld=104, inputs='large')
case("one96-c48-qt1-q127-k80", Rt(64, 48, 0, 1, 96, 0, 1, (2, 5, 4), 1), bq=4, grp=2, heads=5, d=48, lq=127, lk=80, o='wide', form='lse', inputs='heavy')
case("one96-c48-qt2-q193-k96", Rt(64, 48, 0, 2, 96, 0, 1, (2, 5, 4), 1), bq=4, grp=2, heads=5, d=48, lq=193, lk=96, o='wide', vt_ld=104, inputs='heavy')
case("one96-c64s-qt1-q17-k65", Rt(64, 64, 1, 1, 96, 0, 1, (1, 3, 3), 0), bq=3, grp=1, heads=3, d=56, lq=17, lk=65, o='odd', form='acc', inputs='heavy')
case("one96-c64s-qt2-q128-k77", Rt(64, 64, 1, 2, 96, 0, 1, (1, 3, 3), 0), bq=3, grp=1, heads=3, d=56, lq=128, lk=77, o='wide', form='lse', vt_ld=104, inputs='large')
case("one96-c64-qt1-q127-k80", Rt(64, 64, 0, 1, 96, 0, 1, (2, 5, 4), 1), bq=4, grp=2, heads=5, d=64, lq=127, lk=80, o='odd', inputs='heavy')
case("one96-c64-qt2-q193-k96", Rt(64, 64, 0, 2, 96, 0, 1, (2, 5, 4), 1), bq=4, grp=2, heads=5, d=64, lq=193, lk=96, o='odd', form='acc', vt_ld=104, inputs='heavy')
case("w96-walk-c48s-qt1-q127-k65", Rt(64, 48, 1, 1, 96, 1, 2, (1, 8, 128), 1), bq=128, grp=1, heads=8, d=40, lq=127, lk=65, o='odd', form='lse', inputs='heavy')
case("w96-walk-c48s-qt2-q129-k77", Rt(64, 48, 1, 2, 96, 1, 2, (1, 6, 172), 2), bq=172, grp=2, heads=6, d=40, lq=129, lk=77, o='wide', form='lse', inputs='large')
case("w96-walk-c48-qt1-q65-k80", Rt(64, 48, 0, 1, 96, 1, 2, (1, 3, 343), 0), bq=343, grp=343, heads=3, d=48, lq=65, lk=80, o='odd', vt_ld=88, form='lse', inputs='heavy')
case("w96-walk-c48-qt2-q129-k96", Rt(64, 48, 0, 2, 96, 1, 2, (1, 5, 208), 1), bq=208, grp=2, heads=5, d=48, lq=129, lk=96, o='wide', form='lse', inputs='heavy')
case("w96-walk-c64s-qt1-q100-k65", Rt(64, 64, 1, 1, 96, 1, 2, (1, 10, 108), 2), bq=108, grp=4, heads=10, d=56, lq=100, lk=65, o='wide', form='acc', inputs='large')
case("w96-walk-c64s-qt2-q129-k77", Rt(64, 64, 1, 2, 96, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=56, lq=129, lk=77, o='odd', form='acc', inputs='heavy')
case("w96-walk-c64-qt1-q127-k80", Rt(64, 64, 0, 1, 96, 1, 2, (1, 4, 256), 1), bq=256, grp=256, heads=4, d=64, lq=127, lk=80, o='odd', vt_ld=88, form='acc', inputs='heavy')
case("w96-walk-c64-qt2-q129-k96", Rt(64, 64, 0, 2, 96, 1, 2, (1, 12, 86), 2), bq=86, grp=2, heads=12, d=64, lq=129, lk=96, o='wide', form='acc', inputs='large')
# ---- default environment: the edges of the walk (qbw 3 and 8, a last workgroup that breaks early, 2047 | 2048 workgroups), of
# the thresholds (lk 64 | 65 at dqk 64, lk 77 at dqk 96, lq 127 | 128) and the three mappings on heads 3, 5, 6, 10
case("walk-2047-workgroups", Rt(32, 16, 1, 2, 64, 0, 1, (23, 89, 1), 0), bq=1, heads=89, d=8, lq=2817, lk=64, o='odd', grp=1)
case("walk-2048-workgroups", Rt(32, 16, 1, 2, 64, 1, 2, (1, 1024, 1), 2), bq=1, heads=1024, d=8, lq=129, lk=64, o='wide', form='lse', grp=1)
case("walk-qbw3", Rt(32, 32, 1, 2, 64, 1, 3, (1, 3, 343), 0), bq=343, grp=7, heads=3, d=24, lq=257, lk=33, inputs='large')
case("walk-qbw2-of-3-blocks", Rt(32, 16, 0, 2, 64, 1, 2, (2, 5, 140), 1), bq=140, grp=2, heads=5, d=16, lq=300, lk=64, form='acc', inputs='heavy', o='wide')
case("walk-qbw8-of-9-blocks", Rt(32, 16, 1, 2, 64, 1, 8, (2, 911, 1), 0), bq=1, heads=911, d=8, lq=1025, lk=57, grp=1, inputs='heavy')
case("walk-remap1-gx2", Rt(64, 48, 1, 2, 96, 1, 2, (2, 5, 108), 1), bq=108, grp=2, heads=5, d=40, lq=385, lk=77, form='lse', inputs='heavy', o='wide')
case("walk-remap2-h6", Rt(32, 32, 1, 2, 64, 1, 2, (1, 6, 172), 2), bq=172, grp=1, heads=6, d=24, lq=129, lk=64, inputs='large', o='odd')
case("walk-remap0-h3", Rt(64, 48, 1, 1, 96, 1, 2, (1, 3, 683), 0), bq=683, grp=1, heads=3, d=40, lq=70, lk=77, o='odd', inputs='heavy')
case("one-remap1-h3", Rt(64, 48, 1, 2, 64, 0, 1, (2, 3, 4), 1), bq=4, grp=2, heads=3, d=40, lq=250, lk=128, qk='2C', inputs='heavy', o='odd')
case("one-remap1-h5-b12", Rt(96, 80, 1, 1, 64, 0, 1, (2, 5, 12), 1), bq=12, grp=1, heads=5, d=72, lq=100, lk=77, qk='3C', form='acc', inputs='heavy', o='wide')
case("one-remap2-h6", Rt(96, 80, 0, 2, 64, 0, 1, (2, 6, 4), 2), bq=4, grp=2, heads=6, d=80, lq=200, lk=129, inputs='creep', o='odd')
case("one-remap2-h10", Rt(32, 16, 0, 1, 64, 0, 1, (1, 10, 4), 2), bq=4, grp=4, heads=10, d=16, lq=31, lk=200, inputs='spike', o='wide')
case("one-remap0-h5", Rt(160, 160, 0, 2, 64, 0, 1, (2, 5, 3), 0), bq=3, grp=1, heads=5, d=160, lq=130, lk=140, o='wide', inputs='spike')
case("one-remap0-h3-short", Rt(32, 16, 1, 1, 64, 0, 1, (1, 3, 5), 0), bq=5, grp=5, heads=3, d=8, lq=64, lk=3, o='odd')
case("one-c48-k64", Rt(64, 48, 0, 1, 64, 0, 1, (1, 2, 2), 0), bq=2, heads=2, d=48, lq=33, lk=64, grp=1)
case("one-c48-k65", Rt(64, 48, 0, 1, 96, 0, 1, (1, 2, 2), 0), bq=2, heads=2, d=48, lq=33, lk=65, inputs='heavy', grp=1)
case("one-c96-k77", Rt(96, 80, 0, 1, 64, 0, 1, (2, 8, 2), 2), bq=2, heads=8, d=80, lq=96, lk=77, vt_ld=88, inputs='heavy', grp=1, o='odd')
case("one-c48-q127", Rt(64, 48, 1, 1, 64, 0, 1, (2, 8, 2), 2), bq=2, heads=8, d=40, lq=127, lk=130, qk='2C', inputs='heavy', grp=1, o='wide')
case("one-c48-q128", Rt(64, 48, 1, 2, 64, 0, 1, (1, 8, 2), 2), bq=2, heads=8, d=40, lq=128, lk=130, qk='2C', inputs='heavy', grp=1, o='odd')
case("one-c48-creep-6-tiles", Rt(64, 48, 1, 2, 64, 0, 1, (2, 4, 2), 2), bq=2, grp=2, heads=4, d=40, lq=144, lk=321, inputs='creep', form='lse', o='wide')
case("one-c64-creep-rn", Rt(64, 64, 0, 1, 64, 0, 1, (1, 3, 1), 0), bq=1, heads=3, d=64, lq=48, lk=200, inputs='creep', o='wide', grp=1)
case("one-c48s-creep-qt1", Rt(64, 48, 1, 1, 64, 0, 1, (2, 3, 2), 0), bq=2, heads=3, d=40, lq=100, lk=200, inputs='creep', form='acc', grp=1)
case("one-c160-large-5-tiles", Rt(160, 160, 1, 2, 64, 0, 1, (2, 2, 1), 0), bq=1, heads=2, d=152, lq=129, lk=263, inputs='large', vt_ld=272, grp=1)
# ---- kvt128-qt1: 128-key tiles for dqk <= 64
case("qt1-one-c16s-qt1-q1-k1", Rt(32, 16, 1, 1, 128, 0, 1, (1, 1, 1), 0), env=KVT128_QT1, bq=1, grp=1, heads=1, d=8, lq=1, lk=1, o='own', form='acc', inputs='heavy')
case("qt1-one-c16-qt1-q15-k129", Rt(32, 16, 0, 1, 128, 0, 1, (1, 2, 3), 0), env=KVT128_QT1, bq=3, grp=1, heads=2, d=16, lq=15, lk=129, vt_ld=144, o='wide', form='acc', inputs='large')
case("qt1-one-c32s-qt1-q16-k135", Rt(32, 32, 1, 1, 128, 0, 1, (1, 3, 2), 0), env=KVT128_QT1, bq=2, grp=2, heads=3, d=24, lq=16, lk=135, qk='2C', o='odd', form='lse', inputs='spike')
case("qt1-one-c32-qt1-q17-k136", Rt(32, 32, 0, 1, 128, 0, 1, (1, 5, 3), 0), env=KVT128_QT1, bq=3, grp=3, heads=5, d=32, lq=17, lk=136, vt_ld=160, o='own', form='lse', inputs='spike')
case("qt1-one-c48s-qt1-q127-k137", Rt(64, 48, 1, 1, 128, 0, 1, (2, 6, 4), 2), env=KVT128_QT1, bq=4, grp=2, heads=6, d=40, lq=127, lk=137, qk='3C', o='wide', inputs='heavy')
case("qt1-one-c48-qt1-q65-k255", Rt(64, 48, 0, 1, 128, 0, 1, (2, 3, 8), 2), env=KVT128_QT1, bq=8, grp=2, heads=3, d=48, lq=65, lk=255, o='odd', inputs='spike')
case("qt1-one-c64s-qt1-q33-k256", Rt(64, 64, 1, 1, 128, 0, 1, (1, 10, 4), 2), env=KVT128_QT1, bq=4, grp=4, heads=10, d=56, lq=33, lk=256, vt_ld=264, o='odd', form='acc', inputs='heavy')
case("qt1-one-c64-qt1-q64-k128", Rt(64, 64, 0, 1, 128, 0, 1, (1, 5, 6), 0), env=KVT128_QT1, bq=6, grp=1, heads=5, d=64, lq=64, lk=128, qk='2C', o='wide', form='acc', inputs='heavy')
case("qt1-walk-c16s-qt1-q127-k1", Rt(32, 16, 1, 1, 128, 1, 2, (1, 8, 128), 1), env=KVT128_QT1, bq=128, grp=1, heads=8, d=8, lq=127, lk=1, o='odd', vt_ld=16, form='lse')
case("qt1-walk-c16-qt1-q100-k128", Rt(32, 16, 0, 1, 128, 1, 2, (1, 6, 172), 2), env=KVT128_QT1, bq=172, grp=2, heads=6, d=16, lq=100, lk=128, o='wide', form='lse', inputs='large')
case("qt1-walk-c32s-qt1-q65-k13", Rt(32, 32, 1, 1, 128, 1, 2, (1, 3, 343), 0), env=KVT128_QT1, bq=343, grp=343, heads=3, d=24, lq=65, lk=13, o='wide', form='acc', inputs='heavy')
case("qt1-walk-c32-qt1-q127-k127", Rt(32, 32, 0, 1, 128, 1, 2, (1, 5, 208), 1), env=KVT128_QT1, bq=208, grp=2, heads=5, d=32, lq=127, lk=127, o='odd', form='acc', inputs='heavy')
case("qt1-walk-c48s-qt1-q100-k9", Rt(64, 48, 1, 1, 128, 1, 2, (1, 10, 108), 2), env=KVT128_QT1, bq=108, grp=4, heads=10, d=40, lq=100, lk=9, o='odd', vt_ld=24, inputs='large')
case("qt1-walk-c48-qt1-q65-k121", Rt(64, 48, 0, 1, 128, 1, 2, (1, 3, 683), 0), env=KVT128_QT1, bq=683, grp=1, heads=3, d=48, lq=65, lk=121, o='wide', inputs='heavy')
case("qt1-walk-c64s-qt1-q127-k40", Rt(64, 64, 1, 1, 128, 1, 2, (1, 4, 256), 1), env=KVT128_QT1, bq=256, grp=256, heads=4, d=56, lq=127, lk=40, o='odd', form='lse')
case("qt1-walk-c64-qt1-q100-k2", Rt(64, 64, 0, 1, 128, 1, 2, (1, 12, 86), 2), env=KVT128_QT1, bq=86, grp=2, heads=12, d=64, lq=100, lk=2, o='wide', form='lse', inputs='large')
# ---- kvt128-qt2: 128-key tiles for dqk <= 64, and QT = 2 of the <128, 128> class on 64-key tiles
case("qt2-one-c16s-qt2-q128-k257", Rt(32, 16, 1, 2, 128, 0, 1, (1, 1, 1), 0), env=KVT128_QT2, bq=1, grp=1, heads=1, d=8, lq=128, lk=257, o='own', form='acc', inputs='heavy')
case("qt2-one-c16-qt2-q129-k383", Rt(32, 16, 0, 2, 128, 0, 1, (2, 2, 3), 0), env=KVT128_QT2, bq=3, grp=1, heads=2, d=16, lq=129, lk=383, vt_ld=392, o='wide', form='acc', inputs='large')
case("qt2-one-c32s-qt2-q257-k384", Rt(32, 32, 1, 2, 128, 0, 1, (3, 3, 2), 0), env=KVT128_QT2, bq=2, grp=2, heads=3, d=24, lq=257, lk=384, qk='2C', o='odd', form='lse', inputs='spike')
case("qt2-one-c32-qt2-q145-k519", Rt(32, 32, 0, 2, 128, 0, 1, (2, 5, 3), 0), env=KVT128_QT2, bq=3, grp=3, heads=5, d=32, lq=145, lk=519, vt_ld=544, o='own', form='lse', inputs='creep')
case("qt2-one-c48s-qt2-q130-k641", Rt(64, 48, 1, 2, 128, 0, 1, (2, 6, 4), 2), env=KVT128_QT2, bq=4, grp=2, heads=6, d=40, lq=130, lk=641, qk='3C', o='wide', inputs='heavy')
case("qt2-one-c48-qt2-q256-k13", Rt(64, 48, 0, 2, 128, 0, 1, (2, 3, 8), 1), env=KVT128_QT2, bq=8, grp=2, heads=3, d=48, lq=256, lk=13, o='odd', inputs='large')
case("qt2-one-c64s-qt2-q193-k127", Rt(64, 64, 1, 2, 128, 0, 1, (2, 10, 4), 1), env=KVT128_QT2, bq=4, grp=4, heads=10, d=56, lq=193, lk=127, vt_ld=136, o='wide', form='acc', inputs='heavy')
case("qt2-one-c64-qt2-q385-k9", Rt(64, 64, 0, 2, 128, 0, 1, (4, 5, 6), 1), env=KVT128_QT2, bq=6, grp=1, heads=5, d=64, lq=385, lk=9, qk='2C', o='wide', form='acc', inputs='heavy')
case("qt2-walk-c16s-qt2-q129-k1", Rt(32, 16, 1, 2, 128, 1, 2, (1, 8, 128), 1), env=KVT128_QT2, bq=128, grp=1, heads=8, d=8, lq=129, lk=1, o='odd', form='lse')
case("qt2-walk-c16-qt2-q129-k128", Rt(32, 16, 0, 2, 128, 1, 2, (1, 6, 172), 2), env=KVT128_QT2, bq=172, grp=2, heads=6, d=16, lq=129, lk=128, o='odd', form='lse', inputs='large')
case("qt2-walk-c32s-qt2-q129-k13", Rt(32, 32, 1, 2, 128, 1, 2, (1, 3, 343), 0), env=KVT128_QT2, bq=343, grp=343, heads=3, d=24, lq=129, lk=13, o='wide', form='acc', inputs='heavy')
case("qt2-walk-c32-qt2-q129-k127", Rt(32, 32, 0, 2, 128, 1, 2, (1, 5, 208), 1), env=KVT128_QT2, bq=208, grp=2, heads=5, d=32, lq=129, lk=127, o='odd', vt_ld=136, form='acc', inputs='heavy')
case("qt2-walk-c48s-qt2-q129-k9", Rt(64, 48, 1, 2, 128, 1, 2, (1, 10, 108), 2), env=KVT128_QT2, bq=108, grp=4, heads=10, d=40, lq=129, lk=9, o='wide', inputs='large')
case("qt2-walk-c48-qt2-q129-k121", Rt(64, 48, 0, 2, 128, 1, 2, (1, 3, 683), 0), env=KVT128_QT2, bq=683, grp=1, heads=3, d=48, lq=129, lk=121, o='wide', inputs='heavy')
case("qt2-walk-c64s-qt2-q129-k40", Rt(64, 64, 1, 2, 128, 1, 2, (1, 4, 256), 1), env=KVT128_QT2, bq=256, grp=256, heads=4, d=56, lq=129, lk=40, o='odd', form='lse')
case("qt2-walk-c64-qt2-q129-k2", Rt(64, 64, 0, 2, 128, 1, 2, (1, 12, 86), 2), env=KVT128_QT2, bq=86, grp=2, heads=12, d=64, lq=129, lk=2, o='odd', vt_ld=16, form='lse', inputs='large')
case("qt2-one-c128s-q128-k129", Rt(128, 128, 1, 2, 64, 0, 1, (1, 3, 2), 0), env=KVT128_QT2, bq=2, grp=2, heads=3, d=104, lq=128, lk=129, inputs='spike', form='lse', o='wide')
case("qt2-one-c128-q145-k64", Rt(128, 128, 0, 2, 64, 0, 1, (2, 3, 2), 0), env=KVT128_QT2, bq=2, grp=2, heads=3, d=128, lq=145, lk=64, inputs='heavy', form='acc', o='wide')
case("qt2-one-c128s-q257-k200", Rt(128, 128, 1, 2, 64, 0, 1, (3, 3, 2), 0), env=KVT128_QT2, bq=2, grp=2, heads=3, d=120, lq=257, lk=200, inputs='creep', form='lse', o='wide')
case("qt2-walk-c128s-q129-k64", Rt(128, 128, 1, 2, 64, 1, 2, (1, 8, 128), 1), env=KVT128_QT2, bq=128, grp=1, heads=8, d=104, lq=129, lk=64, form='acc', inputs='large', o='odd')
case("qt2-walk-c128-q129-k9", Rt(128, 128, 0, 2, 64, 1, 2, (1, 8, 128), 1), env=KVT128_QT2, bq=128, grp=128, heads=8, d=128, lq=129, lk=9, form='lse', inputs='unit', o='wide')
# ---- I2V_ATTN_WALK=0: walk-sized problems on the one-trip kernels
case("walk0-c48s-text", Rt(64, 48, 1, 2, 96, 0, 1, (2, 8, 128), 1), env=WALK0, bq=128, grp=1, heads=8, d=40, lq=129, lk=77, form='lse', inputs='heavy', o='wide')
case("walk0-c16s-qbw8-sized", Rt(32, 16, 1, 2, 64, 0, 1, (9, 911, 1), 0), env=WALK0, bq=1, heads=911, d=8, lq=1025, lk=57, grp=1, inputs='heavy')
case("walk0-c80-h6", Rt(96, 80, 0, 1, 64, 0, 1, (2, 6, 172), 1), env=WALK0, bq=172, grp=2, heads=6, d=80, lq=70, lk=64, form='acc', inputs='large', o='wide')


# ============================================================================================ a case as the library sees it
def layout(c):
    """where the wrapper's operands of a case lie: dict(C, q_rows, k_rows, qk_ld (row stride of the q and of the k matrix), k_col (k's
    first column), o = (rows, columns, first column) of the output's buffer)"""
    Cc = c["heads"] * c["d"]
    q_rows, k_rows = c["bq"] * c["lq"], c["bq"] // c["grp"] * c["lk"]
    ld = {"own": Cc, "2C": 2 * Cc, "3C": 3 * Cc}[c["qk"]]
    o = {"own": (q_rows, Cc, 0), "wide": (q_rows + 3, Cc + 16, 8), "odd": (q_rows + 3, Cc + 12, 4)}[c["o"]]
    return dict(C=Cc, q_rows=q_rows, k_rows=k_rows, qk_ld=ld, k_col=0 if c["qk"] == "own" else Cc, o=o)


def ask_route(lib, c):
    r = lib.AttnRoute()
    rc = lib.load().i2v_attention_route(c["bq"], c["grp"], c["heads"], c["d"], c["lq"], c["lk"], C.byref(r))
    assert rc == 0, lib.load().i2v_last_error()
    return r.as_dict()


def cases_of(env_name):
    return [c for c in CASES if c["env"] == ENVS[env_name]]


def current_env_name():
    """which of ENVS this process runs under (the switches are read once per process), or None"""
    now = tuple(sorted((k, os.environ[k]) for k in SWITCHES if k in os.environ))
    return next((name for name, env in ENVS.items() if tuple(sorted(env)) == now), None)


if __name__ == "__main__":
    # the routes the library answers for the cases of one environment, as JSON {name: route}; the switches are read once per process,
    # so tests/test_attn_routes.py asks each environment in a child that carries it.  Host arithmetic only: no GPU.
    import json
    if len(sys.argv) != 3 or sys.argv[1] != "--routes" or sys.argv[2] not in ENVS:
        sys.exit(f"usage: python tests/attn_route_cases.py --routes {{{' | '.join(ENVS)}}}")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import i2v_adapter_unofficial_amd as pkg
    assert current_env_name() == sys.argv[2], "run this under the environment it is asked about"
    print(json.dumps({c["name"]: ask_route(pkg._lib, c) for c in cases_of(sys.argv[2])}))
