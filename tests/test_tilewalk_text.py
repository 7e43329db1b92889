"""The tiled query kernels' shared device header (lasgun_amd/csrc/tilewalk.h): the prologue, the tile cursor, the lg_hit writer, the id word and
the optimisation-barrier helper stand ONCE there; the families that measured no slower over it go through it and restate nothing, and the
families that kept their text say so (profiles/tilewalk_account.md).  Device-free: source text only."""
import glob
import os
import re

import tilewalk_text
from tilewalk_text import read

OVER = ("k_layers.hip", "k_paths.hip", "k_features.hip", "k_directions.hip", "k_visibility.hip")
# the files that keep their own text of the prologue and tile loop (and of the record, where they write one), by measurement
KEPT = ("k_query.hip", "k_scan.hip", "k_attributes.hip", "k_view_features.hip", "level0.h", "rq_closest_body.h", "k_lit.hip")
OUTSIDE = ("kcommon.h", "walk.h", "shade.h", "packet.h", "wflevel.h", "k_wavefront.hip", "k_mega.hip", "k_queue.hip", "k_closest.hip", "k_tri_frames.hip", "k_sort.hip",
           "k_lens.hip", "k_probe.hip")
TEXTS = ("claim_tile(", "claim_tile_single(", "copy_to_lds(", "wave_has_work(", "__double_as_longlong", "make_uint4(pk + 1u", "asm volatile")


def test_the_header_holds_each_text_once():
    tilewalk_text.tilewalk_header()


def test_the_adopting_kernels_go_through_it_and_restate_nothing():
    for name in OVER:
        src = read("lasgun_amd", "csrc", name)
        assert '#include "tilewalk.h"' in src and "repeat query_kernel's" not in src, name
        tilewalk_text.over_tilewalk(src)
        assert not re.search(r"\b\w+_bits2\(|\b\w+_opaque\(", tilewalk_text.bare(src).replace("ray_opaque(", "")), name


def test_the_families_that_kept_their_text_say_so_and_nothing_else_restates_it():
    account = read("profiles", "tilewalk_account.md")
    for name in KEPT:
        src = read("lasgun_amd", "csrc", name)
        assert '#include "tilewalk.h"' not in src and "profiles/tilewalk_account.md" in src and "repeat query_kernel's" not in src, name
        assert "claim_tile(P.tile_counter, ntiles, band, bands_left, final)" in src and "if (ntiles == 0u) return; // (uniform: before the LDS copy and its barrier)" in src, name
        assert name in account, name
    csrc = os.path.join(tilewalk_text.ROOT, "lasgun_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "k_*.hip"))):
        name = os.path.basename(path)
        if name in KEPT + OUTSIDE + ("tilewalk.h", "scatter_source.h"):  # (scatter_source.h: the record of level 0's scatter families, kept with level0.h)
            continue
        code = tilewalk_text.bare(open(path).read())
        for text in TEXTS:
            assert text not in code, (name, text)
    assert "tilewalk.h" in read("DESIGN.md")
    for name in OVER:
        assert name in account, name
