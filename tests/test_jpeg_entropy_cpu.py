"""The GPU entropy decoder's scheme, rehearsed on the host (icl_jpeg_coefs_file_host: stage A0 + the schedule of jpeg_huff_gpu.hip as a plain
loop over subsequences, sharing the decode step and the acceptance rules of jpeg_entropy.h) against host stage A.

Every qualifying clean file must be ACCEPTED with coefficients equal to stage A's: a scheme that quietly rejected and fell back would pass
every equality test, so the cap on rejected clean files is zero.  Damaged files are either rejected or accepted with stage A's coefficients."""
import numpy as np
import pytest

from tests.jpeg_entropy_cases import corpus, damaged, is_progressive


@pytest.fixture(scope="module")
def L():
    from imageclust_amd import _lib

    return _lib


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return corpus(tmp_path_factory.mktemp("entropy"))


def test_abi_has_the_entropy_symbols(L):
    lib = L.load()
    for name in ("icl_set_ingest_options", "icl_last_entropy_stats", "icl_jpeg_coefs_files", "icl_jpeg_coefs_file_host"):
        assert hasattr(lib, name), name
    assert (L.ENTROPY_HOST, L.ENTROPY_GPU) == (0, 1)


def test_every_qualifying_file_is_accepted_and_equal(L, files):
    rejected, differ, rounds = [], [], 0
    n_qual = 0
    for p in files:
        got, info = L.jpeg_coefs_file_host(p, 1024)
        if is_progressive(p):
            assert info["state"] == -1, (p, info)  # does not qualify
            continue
        n_qual += 1
        want, _ = L.jpeg_coefs_file_host(p, 0)
        rounds = max(rounds, info["rounds"])
        if info["state"] != 1:
            rejected.append((p, info))
        elif not np.array_equal(got, want):
            differ.append(p)
    print("qualifying files %d, most rounds a workgroup needed %d" % (n_qual, rounds))
    assert n_qual >= 50
    assert not rejected, "clean files rejected: %s" % rejected
    assert not differ, "coefficients differ from stage A: %s" % differ


@pytest.mark.parametrize("sub_bits", [256, 4096])
def test_results_do_not_depend_on_the_subsequence_size(L, files, sub_bits):
    """A quarter and four times the pipeline's size, on every qualifying file (the 1080p and 12 Mpixel ones have the most workgroups)."""
    for p in files:
        if is_progressive(p):
            continue
        got, info = L.jpeg_coefs_file_host(p, sub_bits)
        want, _ = L.jpeg_coefs_file_host(p, 0)
        assert info["state"] == 1 and np.array_equal(got, want), (p, sub_bits, info)


def test_shared_table_file_longer_than_the_launch_count_is_accepted(L, files):
    """Components that share one table pair never re-synchronise in the block-within-MCU index; that index is then not part of the state."""
    big = [p for p in files if "keep_rgb_1920x1080" in p]
    if not big:
        pytest.skip("this Pillow cannot write keep_rgb files")
    got, info = L.jpeg_coefs_file_host(big[0], 1024)
    assert info["nsub"] > 8 * 256, info  # far more workgroups than synchronisation launches
    want, _ = L.jpeg_coefs_file_host(big[0], 0)
    assert info["state"] == 1 and np.array_equal(got, want), info


def test_damaged_files_are_rejected_or_equal(L, tmp_path):
    paths = damaged(tmp_path)
    assert len(paths) >= 35
    n_rej = n_acc = 0
    for p in paths:
        got, info = L.jpeg_coefs_file_host(p, 1024)
        if info["state"] != 1:
            n_rej += 1
            continue
        n_acc += 1
        want, _ = L.jpeg_coefs_file_host(p, 0)  # an accepted file is one stage A reads, with these coefficients
        assert np.array_equal(got, want), p
    print("damaged files: %d rejected, %d accepted and equal" % (n_rej, n_acc))
    assert n_rej > 0
    for name in ("rst_removed.jpg", "rst_duplicated.jpg"):
        _, info = L.jpeg_coefs_file_host(str(tmp_path / name), 1024)
        assert info["state"] == 0, (name, info)
