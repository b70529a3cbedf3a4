"""The cases of tests/test_tattn_routes.py (CPU) and tests/test_tattn_routes_gpu.py: one table of temporal-attention problems
(kernels.temporal_attention -> i2v_temporal_attention_f16), each with the environment it runs under and THE ROUTE IT IS EXPECTED TO
TAKE, written out literally (`i2v_tattn_route`: which of the library's 48 kernel instantiations runs it, and with how many
workgroups).  The shapes are the smallest that reach each instantiation, found on the CPU with the route query and then written down
(`python tests/tattn_route_cases.py --routes ENV` prints what the library answers today for the cases of one environment); a threshold
that moves makes the CPU test fail here instead of moving a case silently to another kernel.

A case is `case(name, route, env=..., n_pixels, frames, heads, head_dim, vt_ld=None, q_ld=None, k_ld=None, o=..., inputs=...)`:
  vt_ld       row stride of V^T [n_pixels, C, vt_ld]; None = pad8(frames).  Columns frames .. vt_ld hold NaN.
  q_ld, k_ld  None: q and k are matrices [rows, C] of their own.  Equal and >= 2 C: column slices [0, C) and [C, 2 C) of ONE
              matrix [rows, q_ld] (2 C: the production form, the q | k projection; 3 C: a q | k | v projection).  Otherwise each the
              first C columns of its own [rows, ld] matrix.
  o           "own": a [rows, C] tensor.  "wide": columns [8, 8 + C) of a poisoned [rows + 3, C + 16] buffer (row stride a multiple
              of 8, 16-byte aligned base).  "odd": columns [4, 4 + C) of a [rows + 3, C + 12] buffer (row stride = 4 mod 8).
              "oddbase": columns [4, 4 + C) of a [rows + 3, C + 16] buffer (row stride a multiple of 8, base 8- but not 16-byte
              aligned).  The last two force the register form at LDS-eligible shapes.
  inputs      "unit" / "large" / "spike": the input family (tests/tattn_bounds.py)
The expected route is L(dqk, dpv, pf, blocks) (LDS-staged form) or R(dqk, dpv, nqt, blocks) (register form).

LDS form: frames <= 16, 2 (48 (C + 8) + C (vt_ld + 8)) <= 65536 bytes, chunks = C / 8 * vt_ld <= 1024, pf = ceil(chunks / 256),
blocks = min(n_pixels, 2048).  Register form: blocks = min(ceil(n_pixels heads / 4), 2048)."""
import ctypes as C
import os
import sys

SWITCHES = ("I2V_TATTN_LDS",)
DEFAULT = ()
LDS_OFF = (("I2V_TATTN_LDS", "0"),)
ENVS = {"default": DEFAULT, "lds0": LDS_OFF}

LDS_FORM, REG_FORM = 0, 1                                   # I2V_TATTN_*_FORM
CLASSES = ((32, 16), (32, 32), (64, 48), (64, 64), (96, 80), (96, 96), (128, 128), (160, 160))
FAMILIES = ("unit", "large", "spike")
OUTPUTS = ("own", "wide", "odd", "oddbase")


def L(dqk, dpv, pf, blocks):
    return dict(form=LDS_FORM, dqk=dqk, dpv=dpv, pf=pf, nqt=0, blocks=blocks)


def R(dqk, dpv, nqt, blocks):
    return dict(form=REG_FORM, dqk=dqk, dpv=dpv, pf=0, nqt=nqt, blocks=blocks)


def pad8(n):
    return (n + 7) // 8 * 8


CASES = []


def case(name, route, env=DEFAULT, *, n_pixels, frames, heads, head_dim, vt_ld=None, q_ld=None, k_ld=None, o="own", inputs="unit"):
    assert all(c["name"] != name for c in CASES), name
    assert o in OUTPUTS and inputs in FAMILIES
    CASES.append(dict(name=name, route=route, env=env, n_pixels=n_pixels, frames=frames, heads=heads, head_dim=head_dim,
                      vt_ld=pad8(frames) if vt_ld is None else vt_ld, q_ld=q_ld, k_ld=k_ld, o=o, inputs=inputs))


# ============================================================================================ the table
# ---- LDS-staged form: four chunk counts per head-dim class.  PF = 4 needs C just under the 64 KiB limit (vt_ld = 16: 384 < C <= 448)
# or a vt_ld wider than pad8(frames).  Frame tails 1, 2, 7, 8, 9, 15, 16; head-dim tails 8, 24, 40, 56, 72, 88, 104, 120, 136, 152;
# heads 1, 2, 3, 5, 9 (the four waves stride the heads by 4).
case("lds-c16-pf1-f1", L(32, 16, 1, 3), n_pixels=3, frames=1, heads=1, head_dim=8)
case("lds-c16-pf2-f15", L(32, 16, 2, 9), n_pixels=9, frames=15, heads=9, head_dim=16)
case("lds-c16-pf3-f16", L(32, 16, 3, 4), n_pixels=4, frames=16, heads=20, head_dim=16, inputs="large")
case("lds-c16-pf4-f9", L(32, 16, 4, 7), n_pixels=7, frames=9, heads=25, head_dim=16)
case("lds-c32-pf1-f2", L(32, 32, 1, 33), n_pixels=33, frames=2, heads=5, head_dim=24)
case("lds-c32-pf2-f8", L(32, 32, 2, 5), n_pixels=5, frames=8, heads=9, head_dim=32, o="wide")
case("lds-c32-pf3-f15", L(32, 32, 3, 6), n_pixels=6, frames=15, heads=14, head_dim=24)
case("lds-c32-pf4-f16", L(32, 32, 4, 3), n_pixels=3, frames=16, heads=13, head_dim=32)
case("lds-c48-pf1-f7", L(64, 48, 1, 40), n_pixels=40, frames=7, heads=1, head_dim=40)
case("lds-c48-pf2-f9-spike", L(64, 48, 2, 12), n_pixels=12, frames=9, heads=5, head_dim=48, inputs="spike")
case("lds-c48-pf3-production", L(64, 48, 3, 10), n_pixels=10, frames=16, heads=8, head_dim=40, q_ld=640, k_ld=640)
case("lds-c48-pf3-large", L(64, 48, 3, 16), n_pixels=16, frames=16, heads=8, head_dim=40, inputs="large", o="wide")
case("lds-c48-pf4-f16", L(64, 48, 4, 3), n_pixels=3, frames=16, heads=9, head_dim=48)
case("lds-c64-pf1-f8", L(64, 64, 1, 17), n_pixels=17, frames=8, heads=2, head_dim=56)
case("lds-c64-pf2-f16", L(64, 64, 2, 5), n_pixels=5, frames=16, heads=3, head_dim=64, q_ld=576, k_ld=576)
case("lds-c64-pf3-f15", L(64, 64, 3, 4), n_pixels=4, frames=15, heads=5, head_dim=64)
case("lds-c64-pf4-f16", L(64, 64, 4, 3), n_pixels=3, frames=16, heads=7, head_dim=64)
case("lds-c80-pf1-f2", L(96, 80, 1, 21), n_pixels=21, frames=2, heads=1, head_dim=72)
case("lds-c80-pf2-f16", L(96, 80, 2, 6), n_pixels=6, frames=16, heads=3, head_dim=80)
case("lds-c80-pf3-f9", L(96, 80, 3, 5), n_pixels=5, frames=9, heads=4, head_dim=80)
case("lds-c80-pf4-f16", L(96, 80, 4, 3), n_pixels=3, frames=16, heads=5, head_dim=80)
case("lds-c96-pf1-f7", L(96, 96, 1, 9), n_pixels=9, frames=7, heads=2, head_dim=88)
case("lds-c96-pf2-f16", L(96, 96, 2, 5), n_pixels=5, frames=16, heads=2, head_dim=96)
case("lds-c96-pf3-f16", L(96, 96, 3, 4), n_pixels=4, frames=16, heads=3, head_dim=96)
case("lds-c96-pf4-f16-d88", L(96, 96, 4, 3), n_pixels=3, frames=16, heads=5, head_dim=88)
case("lds-c96-pf4-vt24", L(96, 96, 4, 3), n_pixels=3, frames=16, heads=3, head_dim=96, vt_ld=24)
case("lds-c128-pf1-f8", L(128, 128, 1, 11), n_pixels=11, frames=8, heads=1, head_dim=104)
case("lds-c128-pf2-f15", L(128, 128, 2, 5), n_pixels=5, frames=15, heads=2, head_dim=128)
case("lds-c128-pf3-f16", L(128, 128, 3, 3), n_pixels=3, frames=16, heads=3, head_dim=120)
case("lds-c128-pf4-vt32", L(128, 128, 4, 3), n_pixels=3, frames=16, heads=2, head_dim=128, vt_ld=32)      # chunks = 1024: the last PF = 4
case("lds-c160-pf1-f1", L(160, 160, 1, 1), n_pixels=1, frames=1, heads=1, head_dim=136)
case("lds-c160-pf2-f16", L(160, 160, 2, 7), n_pixels=7, frames=16, heads=1, head_dim=160)
case("lds-c160-pf3-f9", L(160, 160, 3, 4), n_pixels=4, frames=9, heads=2, head_dim=152)
case("lds-c160-pf4-vt24", L(160, 160, 4, 3), n_pixels=3, frames=16, heads=2, head_dim=160, vt_ld=24)
# n_pixels = 2048 + 5: the first five workgroups fetch a second pixel while they compute the first, the others do not
case("lds-prefetch-2053", L(32, 16, 1, 2048), n_pixels=2053, frames=16, heads=2, head_dim=8)
case("lds-spike-f16", L(32, 32, 2, 12), n_pixels=12, frames=16, heads=5, head_dim=32, inputs="spike")
# ---- register form, one query tile (frames <= 16): C above the LDS limit, more chunks than PF = 4 moves, or an output the LDS
# form's 16-byte row stores cannot take.  Frame tails 1, 2, 7, 8, 9, 15, 16.
case("reg1-c16-f16-h32", R(32, 16, 1, 16), n_pixels=2, frames=16, heads=32, head_dim=16)
case("reg1-c16-gridstride", R(32, 16, 1, 2048), n_pixels=911, frames=2, heads=9, head_dim=8, o="odd")       # 8199 items: a ragged third pass
case("reg1-c32-f7-odd", R(32, 32, 1, 4), n_pixels=5, frames=7, heads=3, head_dim=32, o="odd")
case("reg1-c48-chunks1280", R(64, 48, 1, 12), n_pixels=6, frames=16, heads=8, head_dim=40, vt_ld=32)       # LDS-sized, 1280 chunks
case("reg1-c64-f9", R(64, 64, 1, 16), n_pixels=7, frames=9, heads=9, head_dim=64)
case("reg1-c80-production", R(96, 80, 1, 18), n_pixels=9, frames=16, heads=8, head_dim=80, q_ld=1280, k_ld=1280, inputs="large")
case("reg1-c80-spike", R(96, 80, 1, 24), n_pixels=12, frames=16, heads=8, head_dim=80, inputs="spike")
case("reg1-c96-f1", R(96, 96, 1, 5), n_pixels=3, frames=1, heads=6, head_dim=96)
case("reg1-c128-chunks1152", R(128, 128, 1, 3), n_pixels=4, frames=16, heads=3, head_dim=128, vt_ld=24)    # LDS-sized, 1152 chunks
case("reg1-c160-f8", R(160, 160, 1, 3), n_pixels=3, frames=8, heads=4, head_dim=160, o="wide")
case("reg1-c160-f15-oddbase", R(160, 160, 1, 2), n_pixels=5, frames=15, heads=1, head_dim=136, o="oddbase")
case("reg1-c48-spike-odd", R(64, 48, 1, 15), n_pixels=12, frames=9, heads=5, head_dim=40, o="odd", inputs="spike")
case("reg1-one-pixel", R(32, 32, 1, 1), n_pixels=1, frames=16, heads=3, head_dim=24, o="oddbase")
# ---- register form, two query tiles (frames > 16).  Frame tails 17, 24, 25, 31, 32.
case("reg2-c16-gridstride", R(32, 16, 2, 2048), n_pixels=911, frames=17, heads=9, head_dim=8)              # 8199 items
case("reg2-c32-f24", R(32, 32, 2, 6), n_pixels=7, frames=24, heads=3, head_dim=24)
case("reg2-c48-f25", R(64, 48, 2, 5), n_pixels=9, frames=25, heads=2, head_dim=48, o="wide")
case("reg2-c48-f32-spike", R(64, 48, 2, 15), n_pixels=12, frames=32, heads=5, head_dim=40, inputs="spike")
case("reg2-c64-f31", R(64, 64, 2, 7), n_pixels=5, frames=31, heads=5, head_dim=56)
case("reg2-c80-f32", R(96, 80, 2, 10), n_pixels=5, frames=32, heads=8, head_dim=80, q_ld=1920, k_ld=1920)
case("reg2-c80-f17-d72", R(96, 80, 2, 2), n_pixels=3, frames=17, heads=2, head_dim=72, inputs="large")
case("reg2-c96-f17", R(96, 96, 2, 2), n_pixels=6, frames=17, heads=1, head_dim=96, o="odd")
case("reg2-c96-f31-d88", R(96, 96, 2, 3), n_pixels=4, frames=31, heads=3, head_dim=88)
case("reg2-c128-f32", R(128, 128, 2, 2), n_pixels=4, frames=32, heads=2, head_dim=104)
case("reg2-c128-f25-d120", R(128, 128, 2, 1), n_pixels=1, frames=25, heads=3, head_dim=120)
case("reg2-c160-f25", R(160, 160, 2, 2), n_pixels=5, frames=25, heads=1, head_dim=152)
case("reg2-c160-f24-vt32", R(160, 160, 2, 2), n_pixels=3, frames=24, heads=2, head_dim=160, vt_ld=32)
case("reg2-c32-f17-spike", R(32, 32, 2, 9), n_pixels=12, frames=17, heads=3, head_dim=32, inputs="spike", o="oddbase")
# ---- I2V_TATTN_LDS=0: LDS-eligible shapes on the register kernel
case("off-c48-production", R(64, 48, 1, 20), env=LDS_OFF, n_pixels=10, frames=16, heads=8, head_dim=40, q_ld=640, k_ld=640)
case("off-c16-2053", R(32, 16, 1, 1027), env=LDS_OFF, n_pixels=2053, frames=16, heads=2, head_dim=8)
case("off-c32-f2", R(32, 32, 1, 42), env=LDS_OFF, n_pixels=33, frames=2, heads=5, head_dim=24)
case("off-c64-f15", R(64, 64, 1, 5), env=LDS_OFF, n_pixels=4, frames=15, heads=5, head_dim=64, inputs="large")
case("off-c80-f9", R(96, 80, 1, 5), env=LDS_OFF, n_pixels=5, frames=9, heads=4, head_dim=80, o="wide")
case("off-c96-vt24", R(96, 96, 1, 3), env=LDS_OFF, n_pixels=3, frames=16, heads=3, head_dim=96, vt_ld=24)
case("off-c128-vt32", R(128, 128, 1, 2), env=LDS_OFF, n_pixels=3, frames=16, heads=2, head_dim=128, vt_ld=32)
case("off-c160-f9-spike", R(160, 160, 1, 3), env=LDS_OFF, n_pixels=12, frames=9, heads=1, head_dim=160, inputs="spike")


# ============================================================================================ a case as the library sees it
def layout(c):
    """where the wrappers' operands of a case lie: dict(rows, C, q = (columns of its matrix, first column), k = ..., shared (q and k
    in one matrix), o = (rows, columns, first column) of the output's buffer)"""
    rows, Cc = c["n_pixels"] * c["frames"], c["heads"] * c["head_dim"]
    q_ld, k_ld = c["q_ld"], c["k_ld"]
    shared = q_ld is not None and q_ld == k_ld and q_ld >= 2 * Cc
    q = (q_ld or Cc, 0)
    k = (k_ld or Cc, Cc if shared else 0)
    o = {"own": (rows, Cc, 0), "wide": (rows + 3, Cc + 16, 8), "odd": (rows + 3, Cc + 12, 4), "oddbase": (rows + 3, Cc + 16, 4)}[c["o"]]
    return dict(rows=rows, C=Cc, q=q, k=k, shared=shared, o=o)


BASE = 0x7F0000000000          # fake, well-aligned addresses: one 4 GiB window per operand


def fake_params(lib, c):
    """the i2v_tattn_params that kernels.temporal_attention builds for this case, on fake pointers with the real strides and
    alignments (the route query tests pointers for null and alignment only)"""
    lay = layout(c)
    p = lib.TAttnParams()
    p.q, p.q_row_stride = BASE + 2 * lay["q"][1], lay["q"][0]
    p.k, p.k_row_stride = (BASE if lay["shared"] else BASE + (1 << 32)) + 2 * lay["k"][1], lay["k"][0]
    p.vt, p.vt_ld = BASE + (2 << 32), c["vt_ld"]
    p.o, p.o_row_stride = BASE + (3 << 32) + 2 * lay["o"][2], lay["o"][1]
    p.n_pixels, p.frames, p.heads, p.head_dim = c["n_pixels"], c["frames"], c["heads"], c["head_dim"]
    p.scale = float(c["head_dim"]) ** -0.5
    return p


def ask_route(lib, c):
    p, r = fake_params(lib, c), lib.TAttnRoute()
    rc = lib.load().i2v_temporal_attention_route(C.byref(p), C.byref(r))
    assert rc == 0, lib.load().i2v_last_error()
    return r.as_dict()


def cases_of(env_name):
    return [c for c in CASES if c["env"] == ENVS[env_name]]


def current_env_name():
    """which of ENVS this process runs under (the switch is read once per process), or None"""
    now = tuple(sorted((k, os.environ[k]) for k in SWITCHES if k in os.environ))
    return next((name for name, env in ENVS.items() if tuple(sorted(env)) == now), None)


if __name__ == "__main__":
    # the routes the library answers for the cases of one environment, as JSON {name: route}; the switch is read once per process,
    # so tests/test_tattn_routes.py asks each environment in a child that carries it.  Host arithmetic only: no GPU.
    import json
    if len(sys.argv) != 3 or sys.argv[1] != "--routes" or sys.argv[2] not in ENVS:
        sys.exit(f"usage: python tests/tattn_route_cases.py --routes {{{' | '.join(ENVS)}}}")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import i2v_adapter_unofficial_amd as pkg
    assert current_env_name() == sys.argv[2], "run this under the environment it is asked about"
    print(json.dumps({c["name"]: ask_route(pkg._lib, c) for c in cases_of(sys.argv[2])}))
