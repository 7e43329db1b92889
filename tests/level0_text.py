"""What the source-text tests of the families over level 0's shared bodies (lasgun_amd/csrc/level0.h) assert in common."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def level0_bodies():
    """level0.h holds level 0's three passes ONCE: the one walk, the tile-claim loop, the parked frame, the appends and the finished value."""
    shared = read("lasgun_amd", "csrc", "level0.h")
    assert len(re.findall(r"walk<LDSS, FAST, PRUNE>\(P, ray, false,", shared)) == 1, "one walk, closest hit"
    for text in ("claim_tile(", "claim_tile_single(", "shade_frame(", "(vzero() + value) * 1.0"):
        assert shared.count(text) == 1, text
    assert shared.count("wave_append(P.wf_counts + 1u, ") == 2 and shared.count("shade_lights(") == 1, "one shade body: a reflected and a transmitted child"
    for body in ("void l0_closest_body(const DParams &P, const SRC src)", "void l0_shade_body(const DParams &P, const SRC src)", "void l0_combine_body(const DParams &P, const SRC src)"):
        assert shared.count(body) == 1, body
    assert "level0.h" in read("lasgun_amd", "csrc", "Makefile")
    return shared


def calls_the_bodies(src, closest, shade, combine):
    """A kernel file calls the shared bodies and has no walk, claim loop, frame or append of its own."""
    assert '#include "level0.h"' in src and src.count("l0_closest_body<FAST, LDSS, PRUNE>(P, ") == closest
    assert src.count("l0_shade_body<KIND>(P, ") == shade and src.count("l0_combine_body(P, ") == combine
    for text in ("walk<", "claim_tile", "shade_frame(", "rq_ray_index", "rq_load_ray", "wf_hq[h] = "):
        assert text not in src, text

