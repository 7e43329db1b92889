"""What the source-text tests of the tiled query kernels over the shared device header (lasgun_amd/csrc/tilewalk.h) assert in common."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the text a tiled kernel used to repeat: the claim, the LDS copy and its prologue, the record bits, the id word, the barrier helper
PROLOGUE = ("claim_tile(P.tile_counter, ntiles, band, bands_left, final)", "claim_tile_single(P.tile_counter, ntiles, final)", "copy_to_lds(", "load_accel_image(",
            "wave_has_work(", "if (ntiles == 0u) return", "xcc_id()")
WRITER = ("__double_as_longlong", "out[5] = ", "bits2(b.t, sh.praw.x)", "bits2(INFINITY, 0.0)")
ID_WORD = ("make_uint4(pk + 1u, ", "make_uint4(0u, NO_HIT, NO_HIT, 0xFFFFFFFFu)", "idx - tri_base[b.accel]")
BARRIER = ('asm volatile("" : "+v"(x));',)


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def bare(src):
    return re.sub(r"//[^\n]*", "", src)


def tilewalk_header():
    """tilewalk.h holds the prologue, the cursor, the record writer, the id word and the barrier helper ONCE, the prologue in its order."""
    shared = bare(read("lasgun_amd", "csrc", "tilewalk.h"))
    for text in PROLOGUE + ID_WORD + BARRIER + ("bits2(b.t, sh.praw.x)", "bits2(INFINITY, 0.0)", "__syncthreads();", "TILE_HEADS"):
        assert shared.count(text.replace("if (ntiles == 0u) return", "if (ntiles == 0u) return false")) == 1, text
    assert shared.count("__double_as_longlong") == 2 and shared.count("out[5] = ") == 2, "one bits helper, one hit record, one miss record"
    begin = shared[shared.index("bool begin(const DParams &P, uint32_t tiles)"):shared.index("uint32_t next(const DParams &P, bool &final)")]
    order = [begin.index(t) for t in ("if (ntiles == 0u) return false;", "copy_to_lds(", "__syncthreads();", "load_accel_image(", "if (!wave_has_work(ntiles)) return false;",
                                      "band = LDSS ? xcc_id() : 0u;")]
    assert order == sorted(order), "the empty launch leaves first, every wave reaches the barrier, wave_has_work is asked behind it, the band starts at the XCD"
    store = shared[shared.index("void store_hit(uint4 *out"):shared.index("void store_hit_none(uint4 *out)")]
    assert set(re.findall(r"sh\.(\w+)", store)) == {"praw", "ng", "ns"}, "the record reads praw, ng and ns of Shade (and mat through the id word), nothing else"
    assert set(re.findall(r"sh\.(\w+)", shared[shared.index("uint4 hit_id(const Best &b"):shared.index("uint4 hit_id_none()")])) == {"mat"}
    assert "Counters" not in shared, "the Counters instance stays in the kernel"
    make = read("lasgun_amd", "csrc", "Makefile")
    assert "tilewalk.h" in make[make.index("KHDRS ="):make.index("HOBJS =")]
    for untouched in ("walk.h", "shade.h", "packet.h", "wflevel.h", "kcommon.h", "k_wavefront.hip", "k_mega.hip", "k_queue.hip", "k_closest.hip", "k_tri_frames.hip", "k_sort.hip",
                      "k_lens.hip", "k_probe.hip"):
        assert "tilewalk" not in read("lasgun_amd", "csrc", untouched), untouched
    return shared


def over_tilewalk(src, begin="tw.begin(P)", writer=True, id_word=True, barrier=True):
    """A kernel text goes through the shared prologue and cursor and restates none of it; and, where it writes them, the same of the record,
    the id word and the barrier helper."""
    code = bare(src)
    assert "TileWalk<FAST, LDSS> tw;" in code and "if (!%s) return;" % begin in code and "tw.next(P, final);" in code
    assert "for (bool final = false; !final;) {" in code and "== NO_TILE) break;" in code
    assert "tw.stack, tw.stride, b, tw.scn, cnt, tw.arec)" in code and "Counters cnt = {0, 0, 0, 0, 0, 0, 0, 0, 0};" in code
    for text in PROLOGUE + ("lds_stack", "__syncthreads") + (WRITER if writer else ()) + (ID_WORD if id_word else ()) + (BARRIER if barrier else ()):
        assert text not in code, text
