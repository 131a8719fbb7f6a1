"""Collects the CPU self-tests of tests/footprint.py (a helper module pytest does not collect by name)."""
import footprint
from footprint import *  # noqa: F401,F403
from footprint import (  # noqa: F401
    test_a_planted_change_in_each_region_is_detected_and_located,
    test_clean_copy_has_the_same_layout_and_values_and_zeros_outside,
    test_default_bands_cover_a_tile_of_rows_and_a_mebibyte,
    test_two_dimensional_and_flat_views_report_rows_and_columns,
    test_untouched_buffer_passes_and_view_aliases_the_buffer,
)


def test_every_self_test_of_the_helper_is_collected_here():
    names = {n for n in vars(footprint) if n.startswith("test_")}
    assert names and names <= set(globals()), f"not re-exported: {sorted(names - set(globals()))}"
