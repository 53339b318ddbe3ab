"""snapgpu_align_sam_single_records on the wavefront emulator (tests/emu/): for every option set of
tests/golden/sam_records_single.npz -- -om / -omax / -mpc, -ea, -ae and their combinations -- the call's record list, order included,
equals what the reference CLI wrote, field for field.  The device code that runs here is the code the GPU runs: the align kernels with
secondary results, the adjuster, the record-list kernels (sam_records.h), k_samf_dp8_rec and k_sam_fields_rec.

Test infrastructure only: see tests/test_emu_kernels.py for how the emulated library is swapped in."""
import os
import shutil

import numpy as np
import pytest

from tests import samrec_util as su

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ needed to build the wavefront emulator")


@pytest.fixture(scope="module")
def emu():
    import snap_amd.aligner as al
    from tests.emu.build import build
    path = build()
    saved = (al._lib, al.LIB_PATH)
    os.environ.setdefault("SNAPGPU_EMU_CUS", "4")
    al._lib, al.LIB_PATH = None, path
    try:
        yield al.load_library()
    finally:
        al._lib, al.LIB_PATH = saved


def test_emulated_library_exports_the_records_call(emu):
    assert hasattr(emu, "snapgpu_align_sam_single_records") and hasattr(emu, "snapgpu_align_sam_single_records_device")


@pytest.mark.parametrize("tag", list(su.SETS))
def test_emu_records_equal_the_reference_cli(emu, golden_index, tag):
    z = su.fixture()
    n = z["offsets"].size - 1
    got = su.run_set(golden_index, tag, z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"])
    problems, left_out = su.compare(su.expected(z, tag), got, n)
    print("%s: %d records of %d reads, %d reads left out (reference_history_dependent)" % (tag, got["n_records"], n, left_out))
    assert not problems, problems[:5]
    assert left_out <= 1 + n // 2000


def test_emu_capacity_too_small_then_retry(emu, golden_index):
    """A record capacity below what the batch has: the warning, the needed count, the records that fit exactly as a large enough call
    writes them; a read with more secondary results than the library's first launch has room for (8) is rerun inside the call."""
    z = su.fixture()
    n = 300
    o = z["offsets"][:n + 1]
    args = (golden_index, "ea_om1", z["bases"][:int(o[-1])], z["quals"][:int(o[-1])], o, z["front_clip"][:n], z["data_len"][:n])
    full = su.run_set(*args)
    assert not full["truncated"] and full["n_records"] > n
    assert int(full["n_secondary"].max()) > 8, "the read set no longer has a read whose secondary results outgrow the first stride"
    small = su.run_set(*args, capacity=n // 2, grow=False)
    assert small["truncated"] and small["n_records"] == full["n_records"] and small["rec_read"].size == n // 2
    assert (small["rec_begin"] == full["rec_begin"]).all()
    for f in ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops"):
        assert (small[f] == full[f][:n // 2]).all(), f
    again = su.run_set(*args, capacity=n // 2, grow=True)
    for f in ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops"):
        assert (again[f] == full[f]).all(), f


def test_emu_ae_refuses_a_clipped_read_at_a_contig_end(emu, golden_index):
    su.check_ae_refusal(golden_index)


def test_emu_device_form_equals_the_host_form(emu, golden_index):
    from tests import util
    su.check_device_form(golden_index, util.HipBuffers(emu=True), n=120)
