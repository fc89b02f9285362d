"""Host side of the multi-tile eight-wave GEMM (csrc/gemm.hip), no GPU needed: the grid rule
triad_gemm_w8_workgroups and the rejection rules of triad_gemm_bf16_tiles, which validate before
any launch -> TRIAD_EINVAL (1001). One assertion per rule."""
import os

import pytest

EINVAL = 1001


@pytest.fixture(scope="module")
def lib():
    from triad_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.load()


@pytest.mark.parametrize("tiles,cus,want", [
    (597, 256, 199),    # M = 50,944, N = 768: 3 rounds -> 199 workgroups of 3
    (783, 256, 196),    # M = 66,816, N = 768: 4 rounds -> 196 workgroups, the last ones one tile short
    (2388, 256, 239),   # N = 3072: 10 rounds
    (256, 256, 0),      # one round: the one-tile kernel
    (257, 256, 129),
    (272, 256, 136),
    (1, 256, 0),
])
def test_workgroups_rule(lib, tiles, cus, want):
    assert lib.triad_gemm_w8_workgroups(tiles, cus) == want
    if want:   # same makespan as the dispatcher's rounds, every workgroup has a tile
        rounds = -(-tiles // cus)
        assert want <= cus and want <= tiles and -(-tiles // want) == rounds


def test_workgroups_rejects_non_positive_arguments(lib):
    assert lib.triad_gemm_w8_workgroups(0, 256) == EINVAL
    assert lib.triad_gemm_w8_workgroups(-5, 256) == EINVAL
    assert lib.triad_gemm_w8_workgroups(597, 0) == EINVAL
    assert lib.triad_gemm_w8_workgroups(597, -256) == EINVAL


def test_tiles_entry_point_rejects_bad_arguments(lib):
    fake = 4096  # 16-byte aligned, never dereferenced: validation fails first

    def tiles(A=fake, lda=128, B=fake, ldb=128, M=512, N=256, Kd=128, C=fake, ldc=256, wgs=2, ak=1, bk=1):
        return lib.triad_gemm_bf16_tiles(A, lda, ak, B, ldb, bk, M, N, Kd, None, C, ldc, 0, None, 0, wgs, None)

    # its own rules
    assert tiles(wgs=0) == EINVAL and tiles(wgs=-1) == EINVAL                   # workgroups >= 1
    assert tiles(wgs=3) == EINVAL                                               # workgroups <= tiles (2)
    assert tiles(M=384) == EINVAL                                               # M % 256 (a multiple of 128)
    assert tiles(N=384, ldc=384) == EINVAL                                      # N % 256
    assert tiles(ldc=(1 << 27) + 8) == EINVAL                                   # 4 rows of C within 32 bits
    # every rule of launch()
    assert tiles(M=0) == EINVAL and tiles(N=0) == EINVAL and tiles(Kd=0) == EINVAL
    assert tiles(M=-256) == EINVAL and tiles(N=-256) == EINVAL and tiles(Kd=-64) == EINVAL
    assert tiles(M=200) == EINVAL                                               # M % 128
    assert tiles(N=200, ldc=200) == EINVAL                                      # N % 128
    assert tiles(Kd=96) == EINVAL                                               # Kd % 64
    assert tiles(lda=132) == EINVAL and tiles(ldb=132) == EINVAL                # lda, ldb % 8
    assert tiles(ldc=248) == EINVAL and tiles(ldc=0) == EINVAL                  # ldc < N
    assert tiles(A=None) == EINVAL
    assert tiles(B=None) == EINVAL
    assert tiles(C=None) == EINVAL
    assert tiles(A=fake + 2) == EINVAL and tiles(A=fake + 8) == EINVAL          # A not 16-byte aligned
    assert tiles(B=fake + 2) == EINVAL and tiles(B=fake + 8) == EINVAL          # B not 16-byte aligned
    for ak, bk in ((1, 0), (0, 1), (0, 0)):                                     # in every layout's instantiation
        assert tiles(wgs=0, ak=ak, bk=bk) == EINVAL and tiles(M=384, ak=ak, bk=bk) == EINVAL


def test_form_entry_point_still_has_no_form_5(lib):
    fake = 4096
    assert lib.triad_gemm_bf16_form(fake, 128, 1, fake, 128, 1, 256, 256, 128, None, fake, 256, 0, 5, None) == EINVAL
