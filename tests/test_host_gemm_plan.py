"""CPU (no GPU): the dispatch of the NT GEMM launcher, through uvit_op_gemm_nt_plan.

uvit_gemm_nt_launch plans every launch with one pure function (gemm_nt_plan in csrc/gemm.hip: kernel, rows of the main launch, grid,
rows of the 128x128 tail launch) and uvit_op_gemm_nt_plan reports that plan for any CU count without touching a device.  Here the auto
dispatch is compared with tests/gpu_util.py::nt_auto_plan for every row count up to the largest of a training run, at the CU counts of
the boxes DESIGN.md section 6 names and some smaller ones, and the forced variants and the refused shapes with values derived by hand."""
import ctypes as C

import pytest

from gpu_util import GELU_DG, MODELS, MULAUX, TOKENS, launches, nt_auto_plan, nt_boundary_rows

KERNEL = {"128": 0, "256": 1, "256p": 2, "320": 3}      # uvit_gemm_nt_plan_info.kernel (4 / 5: ring kernel, 128- / 160-row tiles)
PATCH, DGELU = 5, 6
ERR_ARG, ERR_SHAPE = -1, -2


@pytest.fixture(scope="module")
def native():
    from uncertainty_vit_amd import native as n
    n.build()
    n.lib()
    return n


def plan(native, mode, M, N, K, cu=256, row_list=0, ldo=None, **tune):
    """(return code, uvit_gemm_nt_plan_info) of a launch with lda = ldw = K."""
    info = native.GemmNtPlanInfo()
    t = native.Tuning.default(**tune)
    rc = native.lib().uvit_op_gemm_nt_plan(mode, M, N, K, K, K, N if ldo is None else ldo, row_list, C.byref(t), cu, C.byref(info))
    return rc, info


def shapes(model):
    """(N, K, mode) of the Block's six launches and of the patch embedding."""
    return list(launches(model).values()) + [(MODELS[model][0], 768, PATCH)]


@pytest.mark.parametrize("persist", [1, 0])
@pytest.mark.parametrize("cu", [256, 240, 224, 304, 64, 8])
def test_auto_dispatch_is_nt_auto_plan_at_every_row_count(native, cu, persist):
    """nt_variant 3, every launch shape of ViT-B / ViT-L / ViT-H and the patch embedding, every M from 1 to kmax x 197: kernel and
    tail rows are those of nt_auto_plan at this CU count, and the two launches cover the M rows."""
    f, info = native.lib().uvit_op_gemm_nt_plan, native.GemmNtPlanInfo()
    t = native.Tuning.default(nt_persist=persist)
    tref, iref = C.byref(t), C.byref(info)
    cases = 0
    for model, (_, _, kmax) in MODELS.items():
        for N, K, mode in shapes(model):
            for M in range(1, kmax * TOKENS + 1):
                assert f(mode, M, N, K, K, K, N, 0, tref, cu, iref) == 0, (model, N, K, mode, M)
                kern, tail = nt_auto_plan(M, N, K, mode, cu, bool(persist))
                if (info.kernel, info.tail_rows, info.rows) != (KERNEL[kern], tail, M - tail):
                    raise AssertionError(f"{model} N={N} K={K} mode={mode} M={M} at {cu} CUs, nt_persist={persist}: kernel {info.kernel} rows "
                                         f"{info.rows} tail {info.tail_rows}, nt_auto_plan gives {kern} tail {tail}")
            cases += kmax * TOKENS
    print(f"\n[{cu} CUs, nt_persist={persist}] {cases} launches")


def test_default_tuning_is_the_auto_dispatch(native):
    info = native.GemmNtPlanInfo()
    assert native.lib().uvit_op_gemm_nt_plan(GELU_DG, 25216, 3072, 768, 768, 768, 3072, 0, None, 256, C.byref(info)) == 0
    kern, tail = nt_auto_plan(25216, 3072, 768, GELU_DG, 256, True)
    assert (info.kernel, info.tail_rows, info.rows + info.tail_rows) == (KERNEL[kern], tail, 25216)


def test_forced_variants(native):
    """Values derived by hand from the rule at 256 CUs; M = 25216, N = K = 768: 99 x 3 = 297 256-row tiles, 79 x 3 = 237 320-row tiles,
    197 x 6 128x128 tiles, 197 x 3 / 158 x 3 ring tiles.  A forced variant never splits rows."""
    M, N, K = 25216, 768, 768

    def got(variant, persist=1, shape=(M, N, K), mode=0):
        rc, i = plan(native, mode, *shape, nt_variant=variant, nt_persist=persist)
        assert rc == 0
        return i.kernel, i.rows, i.grid, i.tail_rows
    assert got(1, persist=0) == (1, M, 297, 0)
    assert got(1, persist=1) == (2, M, 256, 0)             # 297 tiles > 256 workgroups: persistent, one workgroup per CU
    assert got(5) == (3, M, 237, 0)
    assert got(0) == (0, M, 197 * 6, 0)
    assert got(6) == (4, M, 197 * 3, 0)
    assert got(7) == (5, M, 158 * 3, 0)
    # M < 1024, K % 64 == 32: the ring kernel supports the shape (K >= 64 in steps of 32), the 256-row kernel does not
    assert got(6, shape=(200, 256, 96)) == (4, 200, 2, 0)
    assert got(7, shape=(1300, 512, 160)) == (5, 1300, 9 * 2, 0)
    assert got(6, shape=(200, 256, 64)) == (4, 200, 2, 0)
    assert got(7, shape=(200, 256, 128)) == (5, 200, 2, 0)
    assert got(1, shape=(200, 256, 128)) == (0, 200, 2 * 2, 0)
    # N % 256 != 0: neither does
    assert got(6, shape=(200, 192, 128)) == (0, 200, 2 * 2, 0)


def test_row_list_never_splits(native):
    N, K, mode = launches("vitb")["fc1"]
    for cu in (256, 240):
        M = next(m for m in range(1024, 128 * TOKENS + 1) if nt_auto_plan(m, N, K, mode, cu)[1] > 0)
        rc, i = plan(native, mode, M, N, K, cu=cu)
        assert rc == 0 and i.tail_rows > 0 and i.rows + i.tail_rows == M
        rc, i = plan(native, mode, M, N, K, cu=cu, row_list=1)
        assert rc == 0 and (i.rows, i.tail_rows) == (M, 0) and i.kernel in (1, 2)


@pytest.mark.parametrize("mode", [MULAUX, DGELU])
def test_row_operand_epilogues_are_never_persistent(native, mode):
    """EPI_MULAUX and EPI_DGELU at the fc2-dgrad shape, every k x 197 rows, auto and forced 256-row tiles: never the persistent form,
    which the same launch with the GELU epilogue takes at the largest M."""
    for variant in (3, 1):
        seen = {plan(native, mode, k * TOKENS, 3072, 768, nt_variant=variant)[1].kernel for k in range(1, 129)}
        assert 2 not in seen and {0, 1} <= seen, (variant, seen)
        assert plan(native, GELU_DG, 128 * TOKENS, 3072, 768, nt_variant=variant)[1].kernel == 2


def test_refused_shapes_and_modes(native):
    ok = dict(mode=0, M=2048, N=768, K=768)
    assert plan(native, **ok)[0] == 0
    assert plan(native, **{**ok, "K": 800})[0] == ERR_SHAPE            # K % 64
    for variant, shape in ((1, (2048, 768, 96)), (5, (2048, 768, 96)), (0, (200, 256, 96)), (6, (200, 192, 96)), (6, (100, 256, 96)),
                           (6, (200, 256, 80)), (7, (200, 256, 32))):      # K % 64 where no ring kernel runs, K % 32, K < 64
        assert plan(native, 0, *shape, nt_variant=variant)[0] == ERR_SHAPE, (variant, shape)
    assert plan(native, **{**ok, "N": 772})[0] == ERR_SHAPE            # N % 8
    assert plan(native, **ok, ldo=770)[0] == ERR_SHAPE                 # ldo % 4
    for qkv in (1, 7):
        assert plan(native, **{**ok, "mode": qkv, "N": 256})[0] == ERR_SHAPE       # N % 3
        assert plan(native, **{**ok, "mode": qkv, "N": 2304})[0] == 0
    assert plan(native, **{**ok, "mode": 10})[0] == ERR_ARG
    assert plan(native, **{**ok, "mode": -1})[0] == ERR_ARG
    assert plan(native, **{**ok, "M": 0})[0] == ERR_SHAPE
    assert plan(native, **ok, cu=0)[0] == ERR_ARG
    assert plan(native, **ok, nt_variant=2)[0] == ERR_ARG              # not a variant of uvit_tuning


def test_boundary_rows_cover_every_change_of_the_dispatch():
    """The boundary M are computed, not listed: for every shape they contain 1023 / 1024 and both sides of every change of kernel,
    tile height, persistent form and row split up to the largest M (256 CUs)."""
    for model in MODELS:
        for name, (N, K, mode) in launches(model).items():
            m_max = MODELS[model][2] * TOKENS
            bnd = set(nt_boundary_rows(N, K, mode, m_max))
            assert {1023, 1024} <= bnd
            plans = [None] + [nt_auto_plan(M, N, K, mode) for M in range(1, m_max + 1)]
            for M in range(2, m_max + 1):
                if (plans[M][0], plans[M][1] > 0) != (plans[M - 1][0], plans[M - 1][1] > 0):
                    assert {M - 1, M} <= bnd, (model, name, M)
            assert {"128", "256"} <= {plans[M][0] for M in bnd}, (model, name)
