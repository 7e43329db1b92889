"""The stream contract of the *_device entry points ("enqueue only", on the caller's stream, host tables that may be freed
on return), with the window in which a bug would show held open by construction: the stream is held by a kernel that ends by itself
(stream_program.Blocker: torch.cuda._sleep, calibrated once; 8 x the enqueue time measured on the idle stream in the same test, at least
0.25 s, a failure -- not a skip -- over 2 s), so everything the library enqueued is still behind it when the last call returns
(`not stream.query()`), and every host table has been overwritten with another valid table by then.

  1  every *_device entry point only enqueues: warmed up, timed on the idle stream, then behind the blocker with its host tables
     overwritten on return; the bytes are the synchronous host form's, between intact guard words, planes not asked for at the prefill.
     Path rules and shared lights, whose pointer the library takes as it is, also from PAGE-LOCKED memory: a copy left to the runtime
     reads such a table in stream order, after the overwrite (a pageable one it reads before hipMemcpyAsync returns);
  2  a seeded program of more than 24 calls on one blocked stream, per scene and traversal form: the same family back to back with
     different tables, dependencies through the stream, an output written twice, a ray buffer overwritten behind its reader, small /
     large / small sizes, both query orders, a render between two queries -- after asserting on the references that every pair of tables
     changes at least 10 % of the output words (the rays: hits and misses at least 15 % each, asserted where they are made);
  3  the guards, each shown by the call having DRAINED what was pending on the blocked stream when it returns (`stream.query()`; in (a),
     where the call's own launches follow its wait on that stream, an event recorded on the stream before the call): (a) the first
     larger call of a context grows wf_mem / sort_mem / film_li / gather_li, (b) a ninth stream recycles a context, (c) a setter that
     re-makes the tables, (d) freeing an accel, (e) a host form beside a pending device call.  The stream is held for 8 x the time the
     same action took with nothing pending (a twin stream or accel, in the same test), at least 0.25 s;
  4  four host threads, twelve rounds each of the small mixed calls on a stream each: one shared accel, then an accel per thread.
What a missing guard would do is read a block that was handed on: each guard case synchronises before it touches the library again, so a
missing guard fails an assertion and no kernel runs on such a block."""
import gc
import threading
import time
import weakref

import numpy as np
import pytest

import stream_program as P
from stream_program import G, SMALL, MID, LARGE, Blocker

pytestmark = pytest.mark.gpu

_envs = {}


def env(torch, name="cornell_glass", form="lds"):
    """The scene in the form, built once and shared (every test leaves the accel as it found it)."""
    if (name, form) not in _envs:
        _envs[(name, form)] = P.Env(torch, name, form)
    return _envs[(name, form)]


def timed(call):
    """The host's time for call()."""
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def held_for(rehearsal, what):
    """How long the stream is held for a guard: 8 x the host's time for the SAME action with nothing pending (`rehearsal`, measured on a
    twin in the same test), at least 0.25 s, a failure over 2 s -- so a call that merely takes long cannot look like a call that waited."""
    t = Blocker.seconds_for(rehearsal, what)
    print("%s: %.2f ms with nothing pending, held for %.0f ms" % (what, 1e3 * rehearsal, 1e3 * t))
    return t


def pend(torch, stream, op, seconds):
    """`op` pending behind a blocker of `seconds` on `stream`."""
    torch.cuda.synchronize()
    Blocker.hold(torch, stream, seconds)
    P.enqueue(torch, stream, [op])
    assert not stream.query(), (op.name, "the stream was to be busy: the call waited")


def run_now(torch, stream, ops):
    torch.cuda.synchronize()  # (prefills and uploads ran on the default stream, which does not order against this one)
    P.enqueue(torch, stream, ops)
    stream.synchronize()
    for op in ops:
        op.check("warm-up")
        with torch.cuda.stream(stream):
            op.reset()
    stream.synchronize()


@pytest.fixture(scope="module", autouse=True)
def release_the_shared_accels():
    """The accels this file shares among its cases are freed when its last case is through, not at interpreter exit: the files that run
    after it find the device's memory as they would without it."""
    yield
    _envs.clear()
    gc.collect()
    try:
        import torch
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    except ImportError:
        pass
    G.trim_pool()


# ---- 1: each device form only enqueues -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sorted(P.ENTRY_POINTS))
def test_the_device_form_only_enqueues_and_has_staged_its_host_tables(entry):
    torch = pytest.importorskip("torch")
    e = env(torch)
    ops = P.ENTRY_POINTS[entry](e)
    ops = ops if isinstance(ops, list) else [ops]
    for op in ops:
        if op.alt is not None:
            print("%s: the other table changes %.0f %% of the output words" % (entry, 100 * op.tables_matter()))
    P.behind_a_blocker(torch, torch.cuda.Stream(), ops, entry)


# ---- 2: a program of calls on one blocked stream ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", P.FORMS, ids=["%s-%s" % f for f in P.FORMS])
def test_a_program_of_calls_behind_one_blocker(name, form):
    torch = pytest.importorskip("torch")
    e = env(torch, name, form)
    steps, pairs = P.program(e, seed=20 + len(name))
    assert len(pairs) == 7
    for x, y in pairs:
        f = x.tables_matter()
        assert x.refs() == y.alt and y.refs() == x.alt
        print("%s: the pair's tables change %.0f %% of the output words" % (x.name, 100 * f))
    try:
        P.behind_a_blocker(torch, torch.cuda.Stream(), steps, "program %s %s, %d steps" % (name, form, len(steps)))
    finally:
        G.set_query_order(e.acc, 0)


# ---- 3: the guards ---------------------------------------------------------------------------------------------------------------------------------
GROWTH = {
    # what grows: (warm-up calls that grow everything else to the larger size, the small call, the larger call)
    "wf_mem": lambda e: ([], e.radiance(e.rays(SMALL)), e.radiance(e.rays(LARGE))),
    # (MID, not SMALL: a sorted query of fewer than SORT_MIN_RAYS = 65 rays takes no scratch; the case is about scratch that GROWS)
    "sort_mem": lambda e: ([e.intersect(e.rays(LARGE))], e.intersect(e.rays(MID)), e.intersect(e.rays(LARGE))),
    "film_li": lambda e: ([e.radiance(e.rays(LARGE))], e.capture_rays(e.rays(SMALL), 4), e.capture_rays(e.rays(LARGE), 4)),
    "gather_li": lambda e: ([e.radiance_gather(LARGE, 3, True)], e.radiance_gather(SMALL, 3, False), e.radiance_gather(LARGE, 3, False)),
}


@pytest.mark.parametrize("what", sorted(GROWTH))
def test_guard_a_the_first_larger_call_of_a_context_waits_before_its_buffer_grows(what):
    torch = pytest.importorskip("torch")
    e = P.Env(torch, "cornell_glass", "lds", seed=6)  # an accel of its own: each stream's context is new, its buffers empty
    stream, twin = torch.cuda.Stream(), torch.cuda.Stream()
    assert stream.cuda_stream != twin.cuda_stream
    warm, small, large = GROWTH[what](e)
    order = 1 if what == "sort_mem" else 0

    def prepare(s):
        G.set_query_order(e.acc, 0)
        run_now(torch, s, warm)                   # everything but `what` at the larger size already (unsorted: the sort's scratch stays out of it)
        G.set_query_order(e.acc, order)
        run_now(torch, s, [small])                # ... and `what` at the small size
    try:
        prepare(twin)                             # the rehearsal: the same growth in the twin stream's context, nothing pending
        rehearsal = P.enqueue(torch, twin, [large])
        twin.synchronize()
        large.check((what, "rehearsal"))
        with torch.cuda.stream(twin):
            large.reset()
        prepare(stream)
        pend(torch, stream, small, held_for(rehearsal, what))
        before = torch.cuda.Event()
        before.record(stream)  # (the call's own launches follow its wait on the same stream: what must be through is what was there before it)
        assert not before.query()
        P.enqueue(torch, stream, [large])
        drained = before.query()
        torch.cuda.synchronize()  # (before anything else touches the library: a missing guard fails below, nothing reads a block handed on)
        assert drained, (what, "returned with work pending on the stream: the guard is missing")
        small.check(what)
        large.check(what)
    finally:
        G.set_query_order(e.acc, 0)


def test_guard_b_a_ninth_stream_waits_for_the_context_it_recycles():
    torch = pytest.importorskip("torch")
    n_ctx = P.max_launch_ctxs()
    assert n_ctx == 8
    e = P.Env(torch, "cornell_glass", "lds", seed=3)  # an accel of its own: no context yet
    streams = [torch.cuda.Stream() for _ in range(n_ctx + 2)]
    assert len({s.cuda_stream for s in streams}) == n_ctx + 2
    ops = [e.radiance(e.rays(SMALL)) for _ in streams]
    for s, op in zip(streams[:n_ctx], ops):
        run_now(torch, s, [op])                     # eight contexts, grown
    # the rehearsal: a ninth stream with nothing pending takes the least recently used context, streams[0]'s
    rehearsal = P.enqueue(torch, streams[n_ctx], [ops[n_ctx]])
    torch.cuda.synchronize()
    ops[n_ctx].check("ninth stream, nothing pending")
    seconds = held_for(rehearsal, "a ninth stream")
    busy = streams[1:n_ctx + 1]                     # the eight streams that hold the contexts now
    for s, op in zip(busy, ops[1:n_ctx + 1]):
        with torch.cuda.stream(s):
            op.reset()
    torch.cuda.synchronize()
    for s, op in zip(busy, ops[1:n_ctx + 1]):
        Blocker.hold(torch, s, seconds)
        P.enqueue(torch, s, [op])
    assert not any(s.query() for s in busy), "eight streams were to be busy"
    P.enqueue(torch, streams[0], [ops[0]])          # streams[0] has lost its context: the else branch of ctx_for again
    drained = [s.query() for s in busy]
    torch.cuda.synchronize()
    assert all(drained), ("a call on a ninth stream returned with work pending on the contexts' streams", drained)
    for op in ops[:n_ctx + 1]:
        op.check("ninth stream")
    # a second round over all ten streams, a banded render in the rotation (its band contexts come from the same slots)
    w, h = 2048, 1024
    frame = e._frame(w, h)
    film = e.out(frame.nbytes)
    torch.cuda.synchronize()
    G.set_wf_split(e.acc, 4)
    try:
        for i, (s, op) in enumerate(zip(streams, ops)):
            with torch.cuda.stream(s):
                op.reset()
            P.enqueue(torch, s, [op])
            if i == 4:
                G.capture_subset_device(0, 1, e.acc, w, h, film.ptr, stream=s.cuda_stream)
        torch.cuda.synchronize()
    finally:
        G.set_wf_split(e.acc, 0)
    for op in ops:
        op.check("second round")
    film.check(frame.tobytes(), "the banded render")


SETTERS = {
    # the LDS image in the other form; the leaf records a small mesh's tables were made without (a scene without a mesh has none to
    # make: lg_accel_set_prune re-makes nothing there, so this one runs on the instanced torus); the fast mode's trees, the first time
    "set_node_pairs": ("cornell_glass", "lds", lambda acc: G.set_node_pairs(acc, False)),
    "set_prune": ("instanced", "reference", lambda acc: G.set_prune(acc, True)),
    "set_mode": ("cornell_glass", "lds", lambda acc: G.set_mode(acc, True)),
}


@pytest.mark.parametrize("setter", sorted(SETTERS))
def test_guard_c_a_setter_that_remakes_the_tables_waits(setter):
    torch = pytest.importorskip("torch")
    name, form, call = SETTERS[setter]
    twin = P.Env(torch, name, form, seed=4)
    rehearsal = timed(lambda: call(twin.acc))  # the same re-make (host build, upload, synchronise) on a twin accel, nothing pending
    del twin
    e = P.Env(torch, name, form, seed=4)  # an accel of its own: its tables as lg_accel_from made them
    stream = torch.cuda.Stream()
    op = e.radiance(e.rays(MID))
    run_now(torch, stream, [op])
    pend(torch, stream, op, held_for(rehearsal, setter))
    call(e.acc)
    drained = stream.query()
    torch.cuda.synchronize()
    assert drained, (setter, "returned with a call pending that reads the tables it replaced")
    op.check(setter)
    G.set_mode(e.acc, False)      # (the reference was made by the exact walk)
    with torch.cuda.stream(stream):
        op.reset()
    run_now(torch, stream, [op])  # the same bytes from the re-made tables


def test_guard_d_freeing_an_accel_waits_for_its_pending_call():
    torch = pytest.importorskip("torch")

    def free(env_):
        """Drops the Env's accel and collects; returns a weak reference to the accel."""
        ref = weakref.ref(env_.acc)
        env_.acc = None
        gc.collect()
        return ref

    twin = P.Env(torch, "cornell_glass", "lds", seed=5)
    tstream = torch.cuda.Stream()
    top = twin.radiance(twin.rays(MID))
    run_now(torch, tstream, [top])              # (the twin has a launch context to release, as the accel below has)
    top.run = None
    gone = []
    rehearsal = timed(lambda: gone.append(free(twin)))
    assert gone[0]() is None, "the twin accel was to be collected"
    e = P.Env(torch, "cornell_glass", "lds", seed=5)
    stream = torch.cuda.Stream()
    op = e.radiance(e.rays(MID))
    run_now(torch, stream, [op])
    pend(torch, stream, op, held_for(rehearsal, "lg_accel_free"))
    op.run = None  # (the closure holds the Env)
    ref = free(e)
    drained = stream.query()
    torch.cuda.synchronize()
    assert ref() is None, "the accel was to be collected: lg_accel_free has not run"
    assert drained, "lg_accel_free returned with a call pending that reads the accel's buffers"
    op.check("freed")


def test_guard_e_a_host_form_beside_a_pending_device_call_returns_its_own_bytes():
    torch = pytest.importorskip("torch")
    e = env(torch)
    stream = torch.cuda.Stream()
    op = e.radiance(e.rays(MID))
    rays = e.rays(LARGE)
    want = G.radiance(e.acc, rays).tobytes()
    run_now(torch, stream, [op])
    pend(torch, stream, op, Blocker.FLOOR)
    got = G.radiance(e.acc, rays).tobytes()  # (larger than anything the accel's own stream has seen: its context may grow)
    torch.cuda.synchronize()
    assert got == want
    op.check("beside a host form")


# ---- 4: threads ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [True, False], ids=["one_accel", "an_accel_per_thread"])
def test_four_threads_each_on_a_stream_of_its_own(shared):
    torch = pytest.importorskip("torch")
    threads, rounds = 4, 12
    envs = [env(torch)] * threads if shared else [P.Env(torch, "cornell_glass", "lds", seed=10 + i) for i in range(threads)]
    work = [P.small_mix(e) for e in envs]           # the references: made here, before any thread runs
    streams = [torch.cuda.Stream() for _ in range(threads)]
    torch.cuda.synchronize()
    errors = []

    def body(i):
        try:
            torch.cuda.set_device(0)
            rng = np.random.default_rng(i)
            for r in range(rounds):
                ops = [work[i][j] for j in rng.permutation(len(work[i]))]
                P.enqueue(torch, streams[i], ops)
                streams[i].synchronize()
                for op in ops:
                    op.check(("thread", i, "round", r))
                with torch.cuda.stream(streams[i]):
                    for op in ops:
                        op.reset()
        except BaseException as err:  # noqa: BLE001  (reported by the test's own thread)
            errors.append((i, repr(err)))

    ts = [threading.Thread(target=body, args=(i,)) for i in range(threads)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
