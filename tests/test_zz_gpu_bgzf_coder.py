"""The DEFLATE coder of snap_amd/csrc/bgzf.h on the device, path by path: the cases of tests/test_emu_bgzf_coder.py through the same utility
functions (tests/bgzf_util.py).  Every member is parsed by tests/deflate_util.py, a reader of RFC 1951 that is pinned to zlib by
tests/test_deflate_util.py, and every case asserts from the parsed stream that it reached the path it exists for."""
import pytest

from tests import bgzf_util as bz
from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden_ix():
    return util.load_golden_index()


def test_every_length_and_distance_symbol(golden_ix):
    bz.check_every_symbol(golden_ix)


def test_window_edge(golden_ix):
    bz.check_window_edge(golden_ix)


def test_match_cut_by_the_members_end(golden_ix):
    bz.check_cut_match(golden_ix)


def test_dynamic_blocks_of_fewer_than_64_tokens(golden_ix):
    bz.check_short_members(golden_ix)


def test_crc_slices(golden_ix):
    assert bz.check_crc_slices(golden_ix) >= set(range(1, 201)) | {4095, 4096, 4097, 65279, 65280}


def test_header_run_length_edges(golden_ix):
    bz.check_header_runs(golden_ix)


def test_code_length_code_limited_at_7(golden_ix):
    bz.check_code_length_code_limited(golden_ix)


def test_distance_code_limited_at_15(golden_ix):
    bz.check_distance_code_limited(golden_ix)
