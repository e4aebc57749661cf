"""sf_destroy gives back every byte a handle took, for every creator, on an MI355X.  The cases of
tests/_handle_memory_child.py run in one child process."""
import math

import pytest

from _gpu_child import run_case

pytestmark = pytest.mark.gpu

# What a create .. destroy cycle may leave behind that is not the handle's: the largest shortfall the same child shows
# against the library of the commit before the owned list (SIREN_FIT_LIB=<that build> python tests/_handle_memory_child.py
# handle_memory OUT.json), which freed every buffer by hand - so whatever it leaves is the runtime's own pools, not a leak - plus one
# allocation granule (hipMalloc hands out device memory in 2 MiB blocks).
# NOT YET MEASURED: no MI355X run could be had when this test was written, so the figure stands at 0, the least it can
# be, and the bound is one granule.  A measured figure can only widen it; put it here with the date of the run.
PARENT_SHORTFALL = 0
GRANULE = 2 << 20
SLACK = PARENT_SHORTFALL + GRANULE

CREATORS = ["sf_create", "sf_create+sf_feather_attach", "sf_fourier_create", "sf_wavelet_create", "sf_render_create",
            "sf_wavelet_render_create"]


def test_destroy_returns_what_the_handle_took(tmp_path):
    """In one fresh process, for each of sf_create, sf_fourier_create, sf_wavelet_create, sf_render_create and
    sf_wavelet_render_create: create, sf_set_coords, (training handles) one sf_step of two steps with graph replay on,
    sf_destroy.  The SIREN handle is an auto-format fit of 2^20 pixels that also takes a mask (its scratch moves from
    format 8 to 16), three more steps (longer step tables, a new graph) and sf_kmeans_fit; a second SIREN handle takes
    sf_feather_attach.  After every destroy torch.cuda.mem_get_info() reports the free memory read before that handle's
    create, within SLACK.  The child's first round (the process's first use of each kernel) is not measured."""
    got = run_case("_handle_memory_child.py", "handle_memory", tmp_path=tmp_path, timeout=60)
    cases = [c for c in got["cases"] if c["round"] == 1]
    for c in cases:
        print(c)
    assert [c["creator"] for c in cases] == CREATORS
    siren = cases[0]
    assert siren["format_at_create"] == 8 and siren["format_with_mask"] == 16      # the switch did happen
    for c in cases:
        assert all(math.isfinite(x) for x in c.get("loss", []) + c.get("loss_masked", [])), c      # the steps did run
        assert c["shortfall"] <= SLACK, c
