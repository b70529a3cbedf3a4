"""The cases of tests/test_gemm_routes.py (CPU) and tests/test_gemm_routes_gpu.py: one table of GEMM / conv problems, each with the
switches it runs under, whether the split-K workspace is attached, and THE ROUTE IT IS EXPECTED TO TAKE, written out literally
(`i2v_gemm_route`: which of the library's kernel instantiations runs it).  The shapes are the smallest the planner sends to each
form, found on the CPU with the route query and then written down (`python tests/gemm_route_cases.py --routes ENV` prints what the
library answers today for the cases of one environment); a threshold that moves makes the CPU test fail here instead of moving a case
silently to another kernel.

A case is `case(name, op, route, env=..., ws=..., **problem)`:
  op "gemm": kernels.gemm.  M, N, K and
      bias [1]            a bias vector (every case has one unless it says bias=0)
      res                 a residual;  rowvec="block" (+ rpv = rows per vector) or an int (periodic table of that period)
      epi                 "none" / "gelu" / "geglu";   store "rm" / "perm" (+ frames, hw) / "vt" / "vt_t" (+ vt_len)
      out_scale, ln       (LayerNorm fold), a2 = k_split (dual-source A), wstack = rows of A per stacked weight matrix,
      a_perm = (frames, hw), lo = the precise stream's low halves (with res: the residual carries one, too)
      views = 1           A, residual and output are column slices of wider matrices (lda > K, ldr, ldc > N)
  op "conv": kernels.conv3x3.  n, h, w (input image), cin, cout and stride, up (1: nearest-2x first, 2: folded into the weights),
      size (output size of up = 1), bias, rowvec = images per vector, res, gn (groups of the GroupNorm partials), lo, out_scale, f32
  op "vt":   kernels.project_vt.  T tokens, C channels, K, L keys per batch, bias, ln, pe (period of the positional table)
The expected route is R(family, rows, cols, stages, splits, kps, extra, persistent, generic_tile, vec4); a_mode, epilogue and
store_mode of the record are the problem's own and are checked against it as well."""
import ctypes as C
import os
import sys

SWITCHES = ("I2V_GEMM_BIG", "I2V_GEMM_SPLITK", "I2V_GEMM_SPLIT256", "I2V_GEMM_DEEP", "I2V_GEMM_PERSIST", "I2V_GEMM_4W", "I2V_GEMM_TILE",
            "I2V_CONV_THIN")
# (the children also carry the generic kernel's tuning override: see the generic cases of the table)
DEFAULT = ()
PERSIST = (("I2V_GEMM_PERSIST", "1"), ("I2V_GEMM_TILE", "0"))
NARROW = (("I2V_GEMM_DEEP", "0"), ("I2V_GEMM_SPLIT256", "0"), ("I2V_GEMM_TILE", "1"))
ENVS = {"default": DEFAULT, "persist": PERSIST, "deep0_split256_0": NARROW}

GENERIC, THIN, TILE, DEEP, SPLITK = 0, 1, 2, 3, 4          # I2V_ROUTE_*
FAMILY = {GENERIC: "generic", THIN: "conv_thin", TILE: "big tile", DEEP: "big deep", SPLITK: "big split-K"}
NONE, LNF, HILO, GNS, UPF = 0, 1, 2, 4, 8                   # I2V_EXTRA_*
EPI = {"none": 0, "gelu": 1, "geglu": 2}
STORE = {"rm": 0, "perm": 1, "vt": 2, "vt_t": 3}


def big(family, rows, cols, stages=2, splits=0, kps=0, extra=NONE, persistent=0):
    return dict(family=family, rows=rows, cols=cols, stages=stages, splits=splits, kps=kps, extra=extra, persistent=persistent,
                generic_tile=-1, vec4=-1)


def generic(tile, vec4):
    rows, cols = ((128, 128), (128, 64), (64, 128), (64, 64))[tile]
    return dict(family=GENERIC, rows=rows, cols=cols, stages=0, splits=0, kps=0, extra=NONE, persistent=0, generic_tile=tile, vec4=vec4)


THIN_ROUTE = dict(family=THIN, rows=0, cols=0, stages=0, splits=0, kps=0, extra=NONE, persistent=0, generic_tile=-1, vec4=-1)

CASES = []


def case(name, op, route, env=DEFAULT, ws=True, **o):
    assert all(c["name"] != name for c in CASES), name
    CASES.append(dict(name=name, op=op, route=route, env=env, ws=ws, **o))


# ============================================================================================ the table
# Planner's arithmetic at N = 320 (one column tile): 256-row tiles from 129 tiles of 256 rows (33024 rows), 128-row tiles from 125
# tiles of 128 rows (16000 rows; 16128 = 63 x 256 where M % 256 == 0 is needed).  K = 128 is BIG_MIN_K (two K tiles), K = 192 an odd
# tile count.  M tails: 1, 17 and BM - 1 rows over whole tiles.
# ---- 8-wave kernel, tile form, plain A, 256 rows
case("t256-rm-res", "gemm", big(TILE, 256, 320), M=33024 + 1, N=320, K=128, res=1)
case("t256-rm-rowvec", "gemm", big(TILE, 256, 320), M=33024 + 256, N=320, K=192, rowvec="block", rpv=128, out_scale=0.5)
case("t256-rm-period", "gemm", big(TILE, 256, 320), M=33024 + 17, N=320, K=128, rowvec=16)
case("t256-rm-views", "gemm", big(TILE, 256, 320), M=33024 + 255, N=320, K=128, res=1, views=1)
case("t256-rm-dual", "gemm", big(TILE, 256, 320), M=33024, N=320, K=192, a2=64)
case("t256-perm-res", "gemm", big(TILE, 256, 320), M=33024, N=320, K=128, res=1, store="perm", frames=4, hw=4128)
case("t256-vt", "gemm", big(TILE, 256, 320), M=33024 + 17, N=320, K=128, store="vt", vt_len=64)
case("t256-vt_t", "vt", big(TILE, 256, 320), T=33024, C=320, K=128, L=8256, bias=1)
case("t256-geglu", "gemm", big(TILE, 256, 320), M=33024 + 17, N=320, K=192, epi="geglu", out_scale=0.5)
case("t256-stacked", "gemm", big(TILE, 256, 320), M=33024, N=320, K=128, wstack=11008)
case("t256-a_perm", "gemm", big(TILE, 256, 320), M=33024, N=320, K=128, a_perm=(16, 16))
case("t256-ln-rm", "gemm", big(TILE, 256, 320, extra=LNF), M=33024 + 1, N=320, K=128, ln=1, rowvec=16)
case("t256-ln-perm", "gemm", big(TILE, 256, 320, extra=LNF), M=33024, N=320, K=192, ln=1, store="perm", frames=4, hw=4128)
case("t256-ln-vt_t", "vt", big(TILE, 256, 320, extra=LNF), T=33024, C=320, K=128, L=8256, bias=1, ln=1, pe=16)
case("t256-ln-geglu", "gemm", big(TILE, 256, 320, extra=LNF), M=33024 + 255, N=320, K=128, ln=1, epi="geglu")
case("t256-lo-rm", "gemm", big(TILE, 256, 320, extra=HILO), M=33024 + 17, N=320, K=128, res=1, lo=1)
case("t256-lo-perm", "gemm", big(TILE, 256, 320, extra=HILO), M=33024, N=320, K=128, res=1, lo=1, store="perm", frames=4, hw=4128)
# ---- ... 128 rows
case("t128-rm-res", "gemm", big(TILE, 128, 320), M=16000 + 1, N=320, K=128, res=1)
case("t128-rm-rowvec", "gemm", big(TILE, 128, 320), M=16000 + 128, N=320, K=192, rowvec="block", rpv=64, out_scale=0.5)
case("t128-rm-period", "gemm", big(TILE, 128, 320), M=16000 + 17, N=320, K=128, rowvec=16)
case("t128-rm-views", "gemm", big(TILE, 128, 320), M=16000 + 127, N=320, K=128, res=1, views=1)
case("t128-rm-dual", "gemm", big(TILE, 128, 320), M=16000, N=320, K=192, a2=64)
case("t128-perm-res", "gemm", big(TILE, 128, 320), M=16000, N=320, K=128, res=1, store="perm", frames=4, hw=2000)
case("t128-vt", "gemm", big(TILE, 128, 320), M=16000 + 17, N=320, K=128, store="vt", vt_len=64)
case("t128-vt_t", "vt", big(TILE, 128, 320), T=16000, C=320, K=128, L=4000, bias=1)
case("t128-geglu", "gemm", big(TILE, 128, 320), M=16000 + 17, N=320, K=192, epi="geglu", out_scale=0.5)
case("t128-stacked", "gemm", big(TILE, 128, 320), M=16128, N=320, K=128, wstack=5376)
case("t128-a_perm", "gemm", big(TILE, 128, 320), M=16128, N=320, K=128, a_perm=(16, 16))
case("t128-ln-rm", "gemm", big(TILE, 128, 320, extra=LNF), M=16000 + 1, N=320, K=128, ln=1, rowvec=16)
case("t128-ln-perm", "gemm", big(TILE, 128, 320, extra=LNF), M=16000, N=320, K=192, ln=1, store="perm", frames=4, hw=2000)
case("t128-ln-vt_t", "vt", big(TILE, 128, 320, extra=LNF), T=16000, C=320, K=128, L=4000, bias=1, ln=1, pe=16)
case("t128-ln-geglu", "gemm", big(TILE, 128, 320, extra=LNF), M=16000 + 127, N=320, K=128, ln=1, epi="geglu")
case("t128-lo-rm", "gemm", big(TILE, 128, 320, extra=HILO), M=16000 + 17, N=320, K=128, res=1, lo=1)
case("t128-lo-perm", "gemm", big(TILE, 128, 320, extra=HILO), M=16000, N=320, K=128, res=1, lo=1, store="perm", frames=4, hw=2000)
# ---- ... the persistent walk (I2V_GEMM_PERSIST=1): plain A from one source, whole row tiles
case("p256-rm-res", "gemm", big(TILE, 256, 320, persistent=1), env=PERSIST, M=33024, N=320, K=128, res=1)
case("p256-perm", "gemm", big(TILE, 256, 320, persistent=1), env=PERSIST, M=33024, N=320, K=192, res=1, store="perm", frames=4, hw=4128)
case("p256-vt", "gemm", big(TILE, 256, 320, persistent=1), env=PERSIST, M=33024, N=320, K=128, store="vt", vt_len=64)
case("p256-vt_t", "vt", big(TILE, 256, 320, persistent=1), env=PERSIST, T=33024, C=320, K=128, L=8256, bias=1)
case("p256-geglu", "gemm", big(TILE, 256, 320, persistent=1), env=PERSIST, M=33024, N=320, K=128, epi="geglu")
case("p256-ln-rm", "gemm", big(TILE, 256, 320, extra=LNF, persistent=1), env=PERSIST, M=33024, N=320, K=128, ln=1, rowvec=16)
case("p256-ln-perm", "gemm", big(TILE, 256, 320, extra=LNF, persistent=1), env=PERSIST, M=33024, N=320, K=128, ln=1, store="perm", frames=4, hw=4128)
case("p256-ln-vt_t", "vt", big(TILE, 256, 320, extra=LNF, persistent=1), env=PERSIST, T=33024, C=320, K=192, L=8256, bias=1, ln=1, pe=16)
case("p256-ln-geglu", "gemm", big(TILE, 256, 320, extra=LNF, persistent=1), env=PERSIST, M=33024, N=320, K=128, ln=1, epi="geglu", out_scale=0.5)
case("p128-rm-res", "gemm", big(TILE, 128, 320, persistent=1), env=PERSIST, M=16000, N=320, K=128, res=1)
case("p128-perm", "gemm", big(TILE, 128, 320, persistent=1), env=PERSIST, M=16000, N=320, K=192, res=1, store="perm", frames=4, hw=2000)
case("p128-vt", "gemm", big(TILE, 128, 320, persistent=1), env=PERSIST, M=16000, N=320, K=128, store="vt", vt_len=64)
case("p128-vt_t", "vt", big(TILE, 128, 320, persistent=1), env=PERSIST, T=16000, C=320, K=128, L=4000, bias=1)
case("p128-geglu", "gemm", big(TILE, 128, 320, persistent=1), env=PERSIST, M=16000, N=320, K=128, epi="geglu")
case("p128-ln-rm", "gemm", big(TILE, 128, 320, extra=LNF, persistent=1), env=PERSIST, M=16000, N=320, K=128, ln=1, rowvec=16)
case("p128-ln-perm", "gemm", big(TILE, 128, 320, extra=LNF, persistent=1), env=PERSIST, M=16000, N=320, K=128, ln=1, store="perm", frames=4, hw=2000)
case("p128-ln-vt_t", "vt", big(TILE, 128, 320, extra=LNF, persistent=1), env=PERSIST, T=16000, C=320, K=192, L=4000, bias=1, ln=1, pe=16)
case("p128-ln-geglu", "gemm", big(TILE, 128, 320, extra=LNF, persistent=1), env=PERSIST, M=16000, N=320, K=128, ln=1, epi="geglu", out_scale=0.5)
# (what the walk does not take stays on the one-tile-per-workgroup kernels: ragged M, a second source, the low halves)
case("p256-ragged", "gemm", big(TILE, 256, 320), env=PERSIST, M=33024 + 17, N=320, K=128, res=1)
case("p128-dual", "gemm", big(TILE, 128, 320), env=PERSIST, M=16000, N=320, K=192, a2=64)
case("p128-lo", "gemm", big(TILE, 128, 320, extra=HILO), env=PERSIST, M=16000, N=320, K=128, res=1, lo=1)
# ---- 8-wave kernel, tile form, 3x3 convolution (cin = 64: K = 576, nine K tiles), 320 / 256 / 128 columns
case("c256-320", "conv", big(TILE, 256, 320), n=1, h=182, w=181, cin=64, cout=320, res=1, out_scale=0.5)
case("c128-320-s2", "conv", big(TILE, 128, 320), n=1, h=253, w=252, cin=64, cout=320, stride=2)
case("c256-320-lo", "conv", big(TILE, 256, 320, extra=HILO), n=1, h=182, w=181, cin=64, cout=320, res=1, lo=1)
case("c128-320-lo", "conv", big(TILE, 128, 320, extra=HILO), n=1, h=127, w=126, cin=64, cout=320, res=1, lo=1)
case("c256-320-gn", "conv", big(TILE, 256, 320, extra=GNS), n=9, h=64, w=64, cin=64, cout=320, gn=32, rowvec=3)
case("c128-320-gn", "conv", big(TILE, 128, 320, extra=GNS), n=4, h=64, w=64, cin=64, cout=320, gn=32, rowvec=2)
case("c256-320-fold", "conv", big(TILE, 256, 320, extra=UPF), n=33, h=16, w=16, cin=64, cout=320, up=2)
case("c128-320-fold", "conv", big(TILE, 128, 320, extra=UPF), n=16, h=16, w=16, cin=64, cout=320, up=2)
case("c256-256-up", "conv", big(TILE, 256, 256), n=1, h=91, w=91, cin=64, cout=256, up=1)
case("c128-256-up-odd", "conv", big(TILE, 128, 256), n=1, h=64, w=64, cin=64, cout=256, up=1, size=(127, 127))
case("c256-256-fold", "conv", big(TILE, 256, 256, extra=UPF), n=33, h=16, w=16, cin=64, cout=256, up=2)
case("c128-256-fold", "conv", big(TILE, 128, 256, extra=UPF), n=16, h=16, w=16, cin=64, cout=256, up=2)
case("c256-128-asym", "conv", big(TILE, 256, 128), n=1, h=364, w=362, cin=64, cout=128, stride=2, asym=1)
case("c128-128-rowvec", "conv", big(TILE, 128, 128), n=2, h=100, w=80, cin=64, cout=128, rowvec=1)
case("c256-128-fold", "conv", big(TILE, 256, 128, extra=UPF), n=33, h=16, w=16, cin=64, cout=128, up=2)
case("c128-128-fold", "conv", big(TILE, 128, 128, extra=UPF), n=16, h=16, w=16, cin=64, cout=128, up=2)
# ---- 8-wave kernel, deep pipeline (plain A, a partial round of tiles, 10 .. 63 K tiles): 128 x 128 x 4 stages, 128 x 256 x 3 stages
case("d128-rm-n384", "gemm", big(DEEP, 128, 128, stages=4), M=300, N=384, K=640, res=1, out_scale=0.5)
case("d128-rm-k63", "gemm", big(DEEP, 128, 128, stages=4), M=128, N=128, K=4032, rowvec="block", rpv=32)
case("d128-rm-k11-dual", "gemm", big(DEEP, 128, 128, stages=4), M=200, N=256, K=704, a2=64)
case("d128-perm-k13", "gemm", big(DEEP, 128, 128, stages=4), M=256, N=128, K=832, res=1, store="perm", frames=4, hw=32)
case("d128-vt", "gemm", big(DEEP, 128, 128, stages=4), M=100, N=128, K=640, store="vt", vt_len=64)
case("d128-lo-rm", "gemm", big(DEEP, 128, 128, stages=4, extra=HILO), M=300, N=128, K=704, res=1, lo=1)
case("d128-lo-perm", "gemm", big(DEEP, 128, 128, stages=4, extra=HILO), M=256, N=128, K=640, res=1, lo=1, store="perm", frames=4, hw=32)
case("d256-rm", "gemm", big(DEEP, 128, 256, stages=3), M=4100, N=1024, K=640, res=1, out_scale=0.5)
case("d256-rm-k11-views", "gemm", big(DEEP, 128, 256, stages=3), M=4100, N=1024, K=704, res=1, views=1)
case("d256-perm-k13", "gemm", big(DEEP, 128, 256, stages=3), M=4352, N=1024, K=832, res=1, store="perm", frames=4, hw=544)
case("d256-vt", "gemm", big(DEEP, 128, 256, stages=3), M=4100, N=1024, K=640, store="vt", vt_len=64)
case("d256-lo-rm", "gemm", big(DEEP, 128, 256, stages=3, extra=HILO), M=4100, N=1024, K=640, res=1, lo=1)
case("d256-lo-perm", "gemm", big(DEEP, 128, 256, stages=3, extra=HILO), M=4352, N=1024, K=640, res=1, lo=1, store="perm", frames=4, hw=544)
case("d256-n1280", "gemm", big(DEEP, 128, 256, stages=3), M=6528, N=1280, K=640, res=1)
# ---- 8-wave kernel, split-K + reduce pass (residual, row vector, out_scale and the low halves are the reduce pass's work)
case("s128-plain-k81", "gemm", big(SPLITK, 128, 320, splits=8, kps=11), M=100, N=320, K=5184, res=1, lo=1, out_scale=0.5)
case("s128-plain-rowvec", "gemm", big(SPLITK, 128, 320, splits=5, kps=8), M=128, N=320, K=2560, rowvec="block", rpv=32)
case("s256-plain-k65", "gemm", big(SPLITK, 256, 320, splits=8, kps=9), M=1024, N=1280, K=4160, rowvec="block", rpv=256, out_scale=0.5)
case("s128-conv-k81", "conv", big(SPLITK, 128, 320, splits=8, kps=11), n=2, h=8, w=8, cin=576, cout=320, res=1, lo=1)
case("s256-conv-k90", "conv", big(SPLITK, 256, 320, splits=8, kps=12), n=16, h=16, w=16, cin=640, cout=320, rowvec=1, out_scale=0.5)
# ---- the same problems when the caller attaches no split-K workspace (what a C host that attaches none gets)
case("s128-plain-k81-nows", "gemm", generic(3, 1), ws=False, M=100, N=320, K=5184, res=1, lo=1, out_scale=0.5)
case("s256-plain-k65-nows", "gemm", generic(3, 1), ws=False, M=1024, N=1280, K=4160, rowvec="block", rpv=256, out_scale=0.5)
case("s128-conv-k81-nows", "conv", generic(3, 1), ws=False, n=2, h=8, w=8, cin=576, cout=320, res=1, lo=1)
case("s256-conv-k90-nows", "conv", generic(3, 1), ws=False, n=16, h=16, w=16, cin=640, cout=320, rowvec=1, out_scale=0.5)
# ---- I2V_GEMM_DEEP=0 I2V_GEMM_SPLIT256=0: where the deep and the 256-row split problems go without those forms
case("n-d128-rm-n384", "gemm", generic(1, 1), env=NARROW, M=300, N=384, K=640, res=1, out_scale=0.5)
case("n-d256-n1280", "gemm", big(TILE, 128, 320), env=NARROW, M=6528, N=1280, K=640, res=1)
case("n-deep-level8", "gemm", big(SPLITK, 128, 320, splits=4, kps=10), env=NARROW, M=2048, N=1280, K=2560, res=1)
case("n-s256-plain-k65", "gemm", big(SPLITK, 128, 320, splits=8, kps=9), env=NARROW, M=1024, N=1280, K=4160, rowvec="block", rpv=256, out_scale=0.5)
case("n-s256-conv-k90", "conv", big(SPLITK, 128, 320, splits=8, kps=12), env=NARROW, n=16, h=16, w=16, cin=640, cout=320, rowvec=1, out_scale=0.5)
# ---- the halo-tile kernel of narrow convolutions
case("thin", "conv", THIN_ROUTE, n=2, h=16, w=32, cin=64, cout=4)
case("thin-f32", "conv", THIN_ROUTE, n=1, h=8, w=16, cin=128, cout=3, f32=1, out_scale=0.5)
# ---- the generic kernel: four tiles x two A sources, each with the vector (vec4 = 1) and the element-wise (vec4 = 0) epilogue.
# The tile is the model's choice; 128 x 128 (both sources) and the convolution's 128 x 64 win nowhere in it and run under the
# tuning override I2V_GEMM_TILE alone, which the two child environments therefore carry.
case("g3-plain-v1", "gemm", generic(3, 1), M=70, N=36, K=72, res=1, rowvec="block", rpv=35, out_scale=0.5)
case("g3-plain-v0", "gemm", generic(3, 0), M=70, N=30, K=72, res=1, rowvec=8)
case("g3-plain-gelu", "gemm", generic(3, 1), M=130, N=64, K=64, epi="gelu")
case("g3-plain-geglu-v1", "gemm", generic(3, 1), M=130, N=72, K=136, epi="geglu")
case("g3-plain-geglu-v0", "gemm", generic(3, 0), M=130, N=70, K=136, epi="geglu", out_scale=0.5)
case("g3-plain-perm-lo", "gemm", generic(3, 1), M=128, N=64, K=64, res=1, lo=1, store="perm", frames=4, hw=16)
case("g3-plain-vt", "vt", generic(3, 0), T=192, C=24, K=16, L=6)
case("g3-plain-vt_t", "gemm", generic(3, 0), M=24, N=40, K=16, store="vt_t", vt_len=6)
case("g3-plain-dual-k1", "gemm", generic(3, 1), M=65, N=64, K=128, a2=64)
case("g1-plain-v1", "gemm", generic(1, 1), M=8192 + 1, N=256, K=64, res=1)
case("g1-plain-v0", "gemm", generic(1, 0), M=8192 + 1, N=254, K=64, res=1)
case("g2-plain-v1", "gemm", generic(2, 1), M=1088, N=2048, K=64, res=1)
case("g2-plain-v0", "gemm", generic(2, 0), M=1088, N=2046, K=64, res=1)
case("g3-conv-v1", "conv", generic(3, 1), n=3, h=7, w=5, cin=16, cout=40, up=1, size=(13, 10))
case("g3-conv-v0", "conv", generic(3, 0), n=2, h=9, w=9, cin=8, cout=30, stride=2)
case("g3-conv-f32", "conv", generic(3, 1), n=1, h=8, w=16, cin=32, cout=4, f32=1)
case("g2-conv-v1", "conv", generic(2, 1), n=8, h=64, w=64, cin=8, cout=256)
case("g2-conv-v0", "conv", generic(2, 0), n=8, h=64, w=64, cin=8, cout=254)
case("g0-plain-v1", "gemm", generic(0, 1), env=PERSIST, M=130, N=132, K=64, res=1)
case("g0-plain-v0", "gemm", generic(0, 0), env=PERSIST, M=130, N=130, K=64, res=1)
case("g0-conv-v1", "conv", generic(0, 1), env=PERSIST, n=1, h=12, w=11, cin=16, cout=132)
case("g0-conv-v0", "conv", generic(0, 0), env=PERSIST, n=1, h=12, w=11, cin=16, cout=130)
case("g1-conv-v1", "conv", generic(1, 1), env=NARROW, n=1, h=12, w=11, cin=16, cout=68)
case("g1-conv-v0", "conv", generic(1, 0), env=NARROW, n=1, h=12, w=11, cin=16, cout=66)

# ============================================================================================ a case as the library sees it
def canon(c):
    """the case as one GEMM problem in the library's terms (what the wrapper it runs through makes of it)"""
    o = dict(bias=1, res=0, rowvec=0, rpv=0, epi="none", store="rm", frames=0, hw=0, vt_len=0, out_scale=1.0, ln=0, a2=0, wstack=0,
             a_perm=None, lo=0, views=0, f32=0, gn=0, conv=None)
    o.update({k: v for k, v in c.items() if k not in ("name", "op", "route", "env", "ws")})
    if c["op"] == "vt":
        T, Cc, L = c["T"], c["C"], c["L"]
        natural = Cc % 320 == 0 and L % 4 == 0 and T >= 8192           # kernels.project_vt
        o.update(bias=c.get("bias", 0))
        if natural:
            o.update(M=T, N=Cc, store="vt_t", vt_len=L, rowvec=c.get("pe", 0), rv_transposed=1)
        else:
            assert not (o["bias"] or o["ln"] or c.get("pe")), "the swapped operand order takes a plain projection only"
            o.update(M=Cc, N=T, store="vt", vt_len=L)
        o["natural"] = natural
    elif c["op"] == "conv":
        n, h, w, cin, cout = c["n"], c["h"], c["w"], c["cin"], c["cout"]
        stride, up = c.get("stride", 1), c.get("up", 0)
        if up:
            oh, ow = c.get("size", (2 * h, 2 * w))
        else:
            padsum = 1 if c.get("asym") else 2
            oh, ow = (h + padsum - 3) // stride + 1, (w + padsum - 3) // stride + 1
        o.update(M=n * oh * ow, N=cout, K=(4 if up == 2 else 9) * cin,
                 conv=dict(n=n, h=h, w=w, cin=cin, oh=oh, ow=ow, stride=stride, up=up, asym=int(bool(c.get("asym")))))
        if o["rowvec"]:                                                  # images per vector
            o.update(rpv=o["rowvec"] * oh * ow, rowvec="block")
    o["n_out"] = o["N"] // 2 if o["epi"] == "geglu" else o["N"]
    return o


BASE = 0x7F0000000000          # fake, well-aligned addresses: one 4 GiB window per operand
PTRS = ("a", "w", "c", "residual", "rowvec", "ln_wsum", "c_lo", "residual_lo", "workspace", "gn_partial", "a2", "bias")
VIEW_PAD = 320                 # views = 1: the operand is the column slice [VIEW_PAD, VIEW_PAD + width) of a matrix 2 VIEW_PAD wider


def _ptr(name, skew=0):
    return BASE + (PTRS.index(name) << 32) + skew


def fake_params(lib, c):
    """the i2v_gemm_params that kernels.gemm / conv3x3 / project_vt build for this case, on fake aligned pointers (the route query
    tests pointers for null and alignment only), with the split-K workspace the wrappers attach unless the case says ws=False"""
    o = canon(c)
    p = lib.GemmParams()
    M, N, K = o["M"], o["N"], o["K"]
    pad = 2 * VIEW_PAD if o["views"] else 0
    skew = 2 * VIEW_PAD if o["views"] else 0       # bytes: VIEW_PAD fp16 columns into the wide matrix
    p.M, p.N, p.K = M, N, K
    p.w, p.ldw = _ptr("w"), K
    p.epilogue, p.store_mode, p.out_scale = EPI[o["epi"]], STORE[o["store"]], o["out_scale"]
    if o["bias"]:
        p.bias = _ptr("bias")
    cv = o["conv"]
    if cv:
        p.a, p.lda, p.a_mode = _ptr("a"), cv["cin"], lib.I2V_A_CONV3X3
        p.n_img, p.in_h, p.in_w, p.cin = cv["n"], cv["h"], cv["w"], cv["cin"]
        p.out_h, p.out_w, p.stride, p.upsample, p.asym_pad = cv["oh"], cv["ow"], cv["stride"], cv["up"], cv["asym"]
        p.conv_kblock = 64 if cv["cin"] % 64 == 0 else 0
        p.c, p.ldc, p.c_is_f32 = _ptr("c"), N, o["f32"]
        if cv["up"] == 2:
            p.w_batch_stride, p.rows_per_w = N * K, M // 4
            return p                                  # (kernels.conv3x3 attaches no workspace to the folded form)
    else:
        k1 = o["a2"] if o["a2"] else K
        p.a, p.lda, p.a_mode = _ptr("a", skew), k1 + pad, lib.I2V_A_PLAIN
        if o["a2"]:
            p.a2, p.lda2, p.k_split = _ptr("a2"), K - k1, k1
        if o["wstack"]:
            p.w_batch_stride, p.rows_per_w = N * K, o["wstack"]
        if o["a_perm"]:
            p.a_perm_frames, p.a_perm_hw = o["a_perm"]
        if o["store"] in ("vt", "vt_t"):
            ld = (o["vt_len"] + 7) // 8 * 8
            p.c, p.ldc, p.vt_len, p.vt_ld = _ptr("c"), ld, o["vt_len"], ld
        else:
            p.c, p.ldc = _ptr("c", skew), o["n_out"] + pad
        p.frames, p.hw = o["frames"], o["hw"]
        if o["ln"]:
            p.ln_wsum, p.ln_eps = _ptr("ln_wsum"), 1e-5
    if o["res"]:
        p.residual, p.ldr = _ptr("residual", skew), o["n_out"] + pad
    if o["rowvec"] == "block":
        p.rowvec, p.ld_rowvec, p.rows_per_vec = _ptr("rowvec"), N, o["rpv"]
    elif o["rowvec"]:
        p.rowvec, p.rowvec_period = _ptr("rowvec"), o["rowvec"]
        p.ld_rowvec = o["rowvec"] if o.get("rv_transposed") else N
    if o["lo"]:
        p.c_lo = _ptr("c_lo", skew)
        if o["res"]:
            p.residual_lo = _ptr("residual_lo", skew)
    if c["ws"]:
        need = lib.load().i2v_gemm_workspace_bytes(C.byref(p))
        if need > 0:
            p.workspace, p.workspace_bytes = _ptr("workspace"), need
    if o["gn"]:                                        # (kernels.conv3x3 asks with the workspace attached)
        p.gn_groups = o["gn"]
        if lib.load().i2v_gemm_gn_partial_rows(C.byref(p)) > 0:
            p.gn_partial = _ptr("gn_partial")
    return p


def expected_route(lib, c):
    """the case's literal route as the full record: the problem's own a_mode / epilogue / store_mode beside it"""
    o = canon(c)
    return dict(c["route"], a_mode=lib.I2V_A_CONV3X3 if o["conv"] else lib.I2V_A_PLAIN, epilogue=EPI[o["epi"]], store_mode=STORE[o["store"]])


def ask_route(lib, c):
    p, r = fake_params(lib, c), lib.GemmRoute()
    assert lib.load().i2v_gemm_route(C.byref(p), C.byref(r)) == 0
    return r.as_dict()


def cases_of(env_name):
    return [c for c in CASES if c["env"] == ENVS[env_name]]


def current_env_name():
    """which of ENVS this process runs under (the switches are read once per process), or None"""
    now = tuple(sorted((k, os.environ[k]) for k in SWITCHES if k in os.environ))
    return next((name for name, env in ENVS.items() if tuple(sorted(env)) == now), None)


if __name__ == "__main__":
    # the routes the library answers for the cases of one environment, as JSON {name: route}; the switches are read once per
    # process, so tests/test_gemm_routes.py asks each environment in a child that carries them.  Host arithmetic only: no GPU.
    import json
    if len(sys.argv) != 3 or sys.argv[1] != "--routes" or sys.argv[2] not in ENVS:
        sys.exit(f"usage: python tests/gemm_route_cases.py --routes {{{' | '.join(ENVS)}}}")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import i2v_adapter_unofficial_amd as pkg
    assert current_env_name() == sys.argv[2], "run this under the environment it is asked about"
    print(json.dumps({c["name"]: ask_route(pkg._lib, c) for c in cases_of(sys.argv[2])}))
