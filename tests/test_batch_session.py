"""A batch of filter handles living through scripted sessions, the CPU oracle in lock step (tests/batch_session.py drives
the members with the batched calls and checks each of them stage by stage on inputs read back from the device).

What tests/test_batch*.py leave open: they build fresh handles, run 1-10 steps with one fixed set of filters in one order,
and compare with a standalone twin — the same library on another path.  Here the thread-local staging contexts of
csrc/tdr_host_batch.cpp are reused while k shrinks and grows and two maps alternate on one thread (E, H), every reason of
batch_eligible() flips in both directions inside one array (F), and the per-filter facts the batched step has to keep like
the standalone calls do — the cached pose and scale, maybe_uninit, uniform_scale against scale_frozen, the step count, the
class count, the swap of the state buffers, the generator's position — are changed by standalone calls, map updates and
process-wide switches BETWEEN batched steps (G).  Every batched step is held to the oracle directly.

Each script is a table of events; `test_batch_scripts_are_worth_running` runs them on the oracle alone and asserts that the
inputs exercise what they are meant to.  Events: (fleet, kind, ...) with
  ("set_states", member or members, kind, n or counts) ("init", member) ("solo", member, what) ("switch", name, value) ("window", shape)
  ("map", how, spec, via) ("refuse", what) ("render", members, opts) ("pose", members) ("gmm", members)
  ("step", members, n_targets, sources, own_stream, (batched, standalone), opts)
opts of a step: zero / degenerate / search: member sets; why: {member: (mode, reason)}."""
import numpy as np
import pytest

import batch_session as B
from batch_session import MOTION, _res
from test_handle_session import CW, World, _cloud

COUNTS = (1, 255, 256, 257, 4096, 4097)      # the statistics' and the pose kernels' block edges, in one call (script G)
E_K = (1, 3, 16, 2, 16, 5)
WIDE = (128, 64)             # script F: a window of 8192 bins whose rays stay on the map (36 x 228 = 8208 bins leave it)
FORM_N = 64 * WIDE[0]        # ... at which the default mode takes the integer form from this count on (8192)
REASONS = ("n", "uninit", "gated", "rng", "form_switch", "form_n")


def _names(prefix, k):
    return [f"{prefix}{j}" for j in range(k)]


def _perm(names, seed):
    return [names[i] for i in np.random.default_rng(seed).permutation(len(names))]


# ---- E: membership and staging --------------------------------------------------------------------------------------------
def script_e():
    """16 members on m1 (even: a fixed scale, the uniform-scale table; odd: an unknown scale, a scale draw per particle).
    k per call runs 1, 3, 16, 2, 16, 5 (the staging of tdr_batch_step grows after it shrank), the order is permuted on
    every call, the stream alternates, the sources alternate between host images, a standalone render and a batched render
    that the step reads with no host synchronisation in between (rendered on ANOTHER stream than the step's).  e3 is away
    during the k = 2 call and takes two standalone propagate + update steps meanwhile.  Two refused calls sit in the
    middle.  The counts cross multiples of 256 in both directions, so the resample's block table changes with n_new."""
    e = _names("e", 16)
    ev = [("f", "set_states", e, "equal", [200 + 37 * j for j in range(16)])]
    ev.append(("f", "step", ["e5"], [300], ["host"], False, (1, 0), {}))
    ev.append(("f", "step", ["e9", "e2", "e14"], [-1, 600, 100], ["renderer", "host", "renderer"], True, (3, 0), {}))
    p = _perm(e, 1)
    ev.append(("f", "render", p, dict(stream=True, empty="e7", verify=False)))
    grow = [(-1, 520, 0, 777, 256, 5000)[j % 6] for j in range(16)]     # (0 -> one particle; 5000 -> n_max = 1000)
    ev.append(("f", "step", p, grow, ["batched"] * 16, False, (16, 0), dict(degenerate={"e7"}, zero={"e7"})))
    ev += [("f", "solo", "e3", "propagate"), ("f", "solo", "e3", "update"), ("f", "refuse", "twice"), ("f", "refuse", "shape")]
    ev.append(("f", "step", ["e11", "e0"], [255, 257], ["host", "renderer"], True, (2, 0), {}))
    ev += [("f", "solo", "e3", "propagate"), ("f", "solo", "e3", "update")]
    p = _perm(e, 2)
    ev.append(("f", "render", p, dict(stream=False, empty=None, verify=True)))
    shrink = [(300, -1, 900, 64, 513, 257)[j % 6] for j in range(16)]
    ev.append(("f", "step", p, shrink, [("host", "renderer", "batched")[j % 3] for j in range(16)], True, (16, 0), {}))
    five = ["e12", "e3", "e7", "e0", "e15"]
    ev += [("f", "pose", five), ("f", "gmm", five)]
    ev.append(("f", "step", five, [("adaptive", 450)] * 5, ["host"] * 5, False, (5, 0), {}))
    return ev


# ---- F: eligibility flips ------------------------------------------------------------------------------------------------------
def script_f():
    """Four polar members (and a Cartesian one for the refused call).  batch_eligible() looks at the generator
    (rng_device_capable: configure(0) takes the filter off the reference stream), maybe_uninit with the batch_init_search
    switch, 1 <= n <= 32768, and the form the filter's standalone launch would take.  The form (tdr_su_shape_ok, score_ws):
    tdr_config_shift_uniform(2) makes every launch the integer form; in the default mode 1 it is the integer form only
    with nb * nr >= 8192 bins AND n >= 64 nb — at 36 x 12 the count never flips it (2304 = 64 x 36 matters only once the
    window holds 8192 bins: 36 x 228, whose rays leave this map and leave every weight NaN), so the flip by n is made
    at the window 128 x 64 with u at 8191 / 8192 = 64 x 128 particles for those three rows.
    Every row states the pair and, per member, (mode, the reason it exercises)."""
    all4 = ["big", "u", "g", "c"]

    def why(big, u, g, c):
        return dict(why=dict(big=big, u=u, g=g, c=c))

    ev = [("f", "set_states", ["big", "u", "c", "x"], "equal", [3000, 1500, 1000, 500]), ("f", "init", "g")]
    # F1: g is gated (fixed_scale < 0): its particles may stay without a heading, and the switch is 0
    ev.append(("f", "step", all4, [32768, -1, -1, -1], ["host"] * 4, False, (3, 1),
               why(("B", "n"), ("B", "uninit"), ("S", "gated"), ("B", "rng"))))
    # F2: u holds particles without a heading (switch 0: standalone for this call); c on the device's own noise
    ev += [("f", "set_states", "u", "tenth", 1500), ("f", "solo", "c", "configure0")]
    ev.append(("f", "step", ["c", "g", "big", "u"], [-1, -1, 32769, -1], ["host"] * 4, True, (1, 3),
               dict(search={"u"}, **why(("B", "n"), ("S", "uninit"), ("S", "gated"), ("S", "rng")))))
    # F3: big stands at 32 769; u's search has run; c back on the parity generator
    ev += [("f", "solo", "c", "configure1"), ("f", "refuse", "cart")]
    ev.append(("f", "step", ["u", "big", "c", "g"], [-1, 32768, -1, -1], ["renderer", "host", "host", "renderer"], False, (2, 2),
               why(("S", "n"), ("B", "uninit"), ("S", "gated"), ("B", "rng"))))
    # F4: the search inside the batch: u un-initialised again, g gated — both batched now
    ev += [("f", "switch", "batch_init_search", 1), ("f", "set_states", "u", "tenth", 1500)]
    ev.append(("f", "step", all4, [32769, -1, -1, -1], ["host"] * 4, True, (4, 0),
               dict(search={"u"}, **why(("B", "n"), ("B", "uninit"), ("B", "gated"), ("B", "rng")))))
    # F5: the switch back to 0 straight after the search inside the batch: g standalone again, u batched only because the
    # batched step cleared maybe_uninit as filter_score does; big at 32 769 again, it comes down to a small count
    ev.append(("f", "switch", "batch_init_search", 0))
    ev.append(("f", "step", ["g", "c", "u", "big"], [-1, -1, -1, 2000], ["host"] * 4, False, (2, 2),
               why(("S", "n"), ("B", "uninit"), ("S", "gated"), ("B", "form_switch"))))
    # F6: every launch the integer form: nobody is batched (the standalone calls read batched renders of another stream)
    ev += [("f", "switch", "shift_uniform", 2), ("f", "render", all4, dict(stream=False, empty=None, verify=False))]
    ev.append(("f", "step", all4, [-1] * 4, ["batched", "renderer", "batched", "batched"], True, (0, 4),
               why(("S", "form_switch"), ("S", "form_switch"), ("S", "gated"), ("S", "form_switch"))))
    # F7: the default mode again; u grows to FORM_N for the next row
    ev.append(("f", "switch", "shift_uniform", 1))
    ev.append(("f", "step", ["big", "c", "u", "g"], [-1, -1, FORM_N, -1], ["host"] * 4, False, (3, 1),
               why(("B", "form_switch"), ("B", "form_n"), ("S", "gated"), ("B", "form_switch"))))
    # F8 - F10: 8192 bins: u at FORM_N takes the integer form, at FORM_N - 1 the float form, at FORM_N the integer form
    ev.append(("f", "window", WIDE))
    for nt, mode in ((FORM_N - 1, "S"), (FORM_N, "B"), (-1, "S")):
        ev.append(("f", "step", ["c", "u"], [-1, nt], ["host"] * 2, mode == "B", (2, 0) if mode == "B" else (1, 1),
                   dict(why=dict(c=("B", "rng"), u=(mode, "form_n")))))
    ev.append(("f", "window", (36, 12)))
    ev.append(("f", "step", ["u", "g", "c", "big"], [1500, -1, -1, -1], ["renderer", "host", "host", "host"], False, (3, 1),
               why(("B", "n"), ("B", "form_n"), ("S", "gated"), ("B", "rng"))))
    return ev


# ---- G: state between batched steps ----------------------------------------------------------------------------------------
def script_g():
    """`a` has an unknown scale (a scale draw per particle in its batched steps); then freeze_scale (the uniform-scale
    table in the batch), propagate_freeze(0) (uniform_scale must have dropped: the score stage against a twin that never
    promised anything), set_states("unequal").  The window changes and comes back, the map is replaced through each of its
    four entry points (labels: 6 -> 4 classes, another size and resolution) with a batched step after each, `z` gets an
    all-zero scan and `off` has all but one particle off the map in the same call as healthy members of 1, 255, 256, 257,
    4096 and 4097 particles, and `i` is initialised in mid-run (its search inside the batch, then standalone)."""
    p = _names("p", 6)
    everyone = ["a", "off", "z", "i"] + p
    ev = [("f", "set_states", everyone, "equal", [1200, 900, 800, 700] + list(COUNTS))]
    ev.append(("f", "step", everyone, [-1] * 10, ["host"] * 10, False, (10, 0), {}))
    # (p5 holds 4097 particles, the only one past the one-workgroup pose kernel: listed first, so the records' order is
    # not the order the call works in)
    ev += [("f", "pose", ["p5", "a", "p0", "p4"]), ("f", "solo", "a", "freeze")]
    ev.append(("f", "step", ["p0", "a", "z"], [-1, -1, 500], ["host", "renderer", "host"], True, (3, 0), {}))
    ev += [("f", "pose", ["a", "z"]), ("f", "solo", "a", "propagate_freeze0")]
    ev.append(("f", "step", ["a", "p1", "i"], [-1] * 3, ["host"] * 3, False, (3, 0), {}))
    ev.append(("f", "set_states", "a", "unequal", 1000))
    ev.append(("f", "step", ["p2", "a"], [-1, -1], ["renderer", "host"], True, (2, 0), {}))
    ev.append(("f", "window", (25, 16)))
    ev.append(("f", "step", ["z", "a", "p3"], [800, -1, -1], ["host", "renderer", "host"], False, (3, 0), {}))
    ev += [("f", "window", (36, 12)), ("f", "set_states", "off", "offmap", 900)]
    walk = [COUNTS[(j + 1) % 6] for j in range(6)]
    ev.append(("f", "step", ["off"] + p + ["z", "a"], [-1] + walk + [-1, -1], ["host"] * 9, True, (9, 0),
               dict(zero={"z"}, degenerate={"z", "off"})))
    ev.append(("f", "set_states", "off", "equal", 900))
    walk = [COUNTS[(j + 2) % 6] for j in range(6)]
    ev.append(("f", "step", p + ["off"], walk + [-1], ["host"] * 7, False, (7, 0), {}))
    ev += [("f", "switch", "batch_init_search", 1), ("f", "init", "i")]
    ev.append(("f", "step", ["a", "i", "p1"], [-1, 1300, -1], ["host"] * 3, True, (3, 0), dict(search={"i"})))
    ev.append(("f", "switch", "batch_init_search", 0))
    ev.append(("f", "step", ["i", "a"], [-1, -1], ["host"] * 2, False, (1, 1), dict(why=dict(i=("S", "gated")))))
    # process-wide switches between batched steps: the dense records, then the generator without its stretches
    ev += [("f", "switch", "compact", 0), ("f", "step", ["p2", "a", "z"], [-1, 1400, -1], ["host", "host", "renderer"], True, (3, 0), {})]
    ev += [("f", "switch", "compact", 1), ("f", "switch", "mt_stretches", 0),
           ("f", "step", ["z", "p3", "a"], [-1, -1, 1000], ["host"] * 3, False, (3, 0), {}), ("f", "switch", "mt_stretches", 1)]
    small = ["a", "z", "p0", "off"]
    for how, spec, via in (("maps", "m1b", "a"), ("labels", "m2", "z"), ("incremental", "m2b", "a"), ("patch", "m2c", "p0")):
        ev.append(("f", "map", how, spec, via))
        ev.append(("f", "step", small, [-1] * 4, ["host", "renderer", "host", "host"], how in ("maps", "incremental"), (4, 0), {}))
    return ev


# ---- H: two fleets on one thread ---------------------------------------------------------------------------------------------
def script_h():
    """A fleet of 16 on m1 (36 x 12) and a fleet of 2 on m2 (4 classes, 25 x 16) share the thread's staging contexts; their
    step, render and pose calls alternate.  A steps 3 members, B's needs are smaller than what A left behind, then A grows
    to 16 past both."""
    a, b = _names("a", 16), _names("b", 2)
    ev = [("A", "set_states", a, "equal", [300 + 23 * j for j in range(16)]), ("B", "set_states", b, "equal", [400, 500])]
    three = ["a4", "a9", "a1"]
    ev += [("A", "step", three, [-1, 500, 200], ["host"] * 3, False, (3, 0), {}), ("A", "pose", three),
           ("A", "render", three, dict(stream=False, empty=None, verify=True))]
    ev += [("B", "render", b, dict(stream=True, empty=None, verify=False)),
           ("B", "step", b, [-1, 300], ["batched"] * 2, True, (2, 0), {}),
           ("B", "pose", ["b0", "idle", "b1"])]        # (idle: a handle that never got particles — zeros, no device work)
    p = _perm(a, 3)
    ev += [("A", "render", p, dict(stream=True, empty=None, verify=False)),
           ("A", "step", p, [(-1, 600, 257)[j % 3] for j in range(16)], ["batched"] * 16, False, (16, 0), {}), ("A", "pose", p)]
    ev += [("B", "step", b[::-1], [-1, -1], ["host", "renderer"], False, (2, 0), {}), ("B", "pose", b[::-1])]
    five = ["a0", "a15", "a7", "a8", "a2"]
    ev += [("A", "step", five, [-1] * 5, ["renderer", "host", "host", "batched", "host"], True, (5, 0), {}), ("B", "pose", b),
           ("B", "step", ["b0", "idle", "b1"], [450, -1, -1], ["renderer", "host", "host"], True, (2, 1),
            dict(why=dict(idle=("S", "n"))))]         # (no particles: n >= 1 fails, the standalone calls return at once)
    return ev


SCRIPTS = {"E": script_e, "F": script_f, "G": script_g, "H": script_h}
SWITCHES = {
    "shift_uniform": lambda L, v: L.tdr_config_shift_uniform(int(v)),
    "batch_init_search": lambda L, v: L.tdr_config_tuning(b"batch_init_search", int(v)),
    "init_device": lambda L, v: L.tdr_config_tuning(b"init_device", int(v)),
    "compact": lambda L, v: L.tdr_config_compact(int(v)),
    "mt_stretches": lambda L, v: L.tdr_config_tuning(b"mt_stretches", int(v)),
}


def _fleets(oracle, name, handle):
    w = World.get(oracle)

    def member(nm, n_max, seed, j=0, **kw):
        return dict(name=nm, n_max=n_max, seed=seed, params=w.params(class_weights=CW[j % 6:] + CW[:j % 6], **kw))

    if name == "E":
        ms = [member(f"e{j}", 1000, 101 + j, j, fixed_scale=1.25 if j % 2 == 0 else -1.0) for j in range(16)]
        return w, {"f": B.Fleet(oracle, w.m1, ms, handle, name="E")}
    if name == "F":
        ms = [member("big", 33_000, 211, fixed_scale=1.25), member("u", FORM_N + 96, 212, 1, fixed_scale=1.25),
              member("g", 1500, 213, 2), member("c", 1200, 214, 3, fixed_scale=1.25),
              dict(member("x", 600, 215, 4), cart=True)]
        return w, {"f": B.Fleet(oracle, w.m1, ms, handle, name="F", cart_spec=w.m1c)}
    if name == "G":
        ms = [member("a", 1500, 311), member("off", 1000, 312, 1, fixed_scale=1.25), member("z", 1000, 313, 2, fixed_scale=1.25),
              member("i", 1500, 314, 3)]
        ms += [member(f"p{j}", 4200, 320 + j, j, fixed_scale=1.25) for j in range(6)]
        return w, {"f": B.Fleet(oracle, w.m1, ms, handle, name="G")}
    ma = [member(f"a{j}", 800, 401 + j, j, fixed_scale=1.25 if j % 2 else -1.0) for j in range(16)]
    mb = [member(f"b{j}", 700, 451 + j, j, fixed_scale=-1.0 if j else 1.25) for j in range(2)] + [member("idle", 300, 460)]
    return w, {"A": B.Fleet(oracle, w.m1, ma, handle, name="H.A"), "B": B.Fleet(oracle, w.m2, mb, handle, shape=(25, 16), name="H.B")}


def run(oracle, name, handle):
    """Runs script `name`; returns the fleets.  Process-wide switches are put back whatever happens."""
    w, fleets = _fleets(oracle, name, handle)
    sw = {"batch_init_search": 0, "shift_uniform": 1}      # the mirror of the two switches eligibility looks at
    L, saved = None, {}
    if handle:
        from top_down_renderer_amd import _lib
        L = _lib.load()
        saved = {"shift_uniform": L.tdr_config_shift_uniform(-1), "batch_init_search": L.tdr_config_tuning(b"batch_init_search", -1),
                 "init_device": L.tdr_config_tuning(b"init_device", -1), "compact": L.tdr_config_compact(-1),
                 "mt_stretches": L.tdr_config_tuning(b"mt_stretches", -1)}
        assert (saved["shift_uniform"], saved["batch_init_search"]) == (1, 0), saved
    try:
        for i, e in enumerate(SCRIPTS[name]()):
            fl, kind = fleets[e[0]], e[1]
            tag = f"#{i} {e[:4]}"
            if kind == "set_states":
                several = isinstance(e[2], list)
                for j, m in enumerate(e[2] if several else [e[2]]):
                    s = fl.ses[m]
                    st = _cloud(w, e[4][j] if several else e[4], 100 + i + 1000 * j, e[3])
                    oracle.shift_init(st, *s.spec.center)      # (the clouds are drawn around the pose on m1, centre (0, 0))
                    s.set_states(st, f"#{i} set_states {m} {e[3]}")
                    fl.uninit[m] = bool((st["have_init"] == 0).any())
            elif kind == "init":
                if L:
                    SWITCHES["init_device"](L, 1)
                fl.ses[e[2]].initialize(tag)
                fl.uninit[e[2]] = True                          # (no heading prior: every particle awaits the search)
            elif kind == "solo":
                s, what = fl.ses[e[2]], e[3]
                if what == "propagate":
                    s.propagate(*MOTION, label=tag)
                elif what == "update":
                    s.update(_res(fl.k), label=tag)
                    s.records[-1].update(call=None, want_search=False, mode="solo", why=None, zero=False)
                    fl.scored(e[2])
                    fl.k += 1
                elif what == "freeze":
                    s.freeze(tag)
                elif what == "propagate_freeze0":
                    s.propagate(*MOTION, freeze=0, label=tag)
                elif what in ("configure0", "configure1"):
                    s.configure(int(what[-1]), 1, tag)
                else:
                    raise AssertionError(e)
            elif kind == "switch":
                sw[e[2]] = e[3]
                if L:
                    SWITCHES[e[2]](L, e[3])
            elif kind == "window":
                fl.window(e[2], tag)
            elif kind == "map":
                fl.new_map(getattr(w, e[3]), e[2], e[4], patch=w.patch if e[2] == "patch" else None, tag=tag)
            elif kind == "refuse":
                fl.refuse(e[2], tag)
            elif kind == "render":
                fl.render(e[2], tag=tag, **e[3])
            elif kind == "pose":
                fl.pose(e[2], stream=i % 2 == 0, tag=tag)
            elif kind == "gmm":
                fl.gmm(e[2], stream=i % 2 == 0, tag=tag)
            elif kind == "step":
                fl.step(e[2], e[3], e[4], e[5], e[6], sw, tag=tag, **e[7])
                fl.calls[-1]["event"] = i
            else:
                raise AssertionError(f"unknown event {e}")
    finally:
        if L:
            for key, v in saved.items():
                SWITCHES[key](L, v)
    return fleets


# ---- the scripts on the oracle alone ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dry(oracle):
    return {name: run(oracle, name, handle=False) for name in SCRIPTS}


def _flips(seq):
    return {a + b for a, b in zip(seq, seq[1:]) if a != b}


def test_batch_scripts_are_worth_running(oracle, dry):
    """Conditions on the INPUTS, met by the oracle alone."""
    # -- every member step but the designated ones is healthy; the search steps do search
    want_deg = {"E": {"E.e7"}, "F": set(), "G": {"G.z", "G.off"}, "H": set()}
    for name, fleets in dry.items():
        deg = set()
        for fl in fleets.values():
            for s in fl.ses.values():
                for r in s.records:
                    tag = (name, s.name, r["label"], {k: r[k] for k in ("n", "n_new", "good", "distinct", "search")})
                    if r["degenerate"]:
                        deg.add(s.name)
                        continue
                    assert r["good"] > 0.5, tag
                    if r["n"] >= 20 and r["n_new"] >= 20:
                        assert r["distinct"] >= r["n_new"] / 20, tag
                    if r["want_search"]:
                        assert r["search"] >= 0.1, tag
        assert deg == want_deg[name], (name, deg)
    assert sum(r["degenerate"] for r in dry["G"]["f"].ses["z"].records) == 1
    assert sum(r["degenerate"] for r in dry["G"]["f"].ses["off"].records) == 1
    assert any(r["want_search"] for r in dry["F"]["f"].ses["u"].records) and any(r["want_search"] for r in dry["G"]["f"].ses["i"].records)
    # -- every event that is not a step is followed by a batched step (of its fleet: any) within four events
    for name, make in SCRIPTS.items():
        table = make()
        assert table[-1][1] == "step", name
        for i, e in enumerate(table):
            if e[1] != "step":
                assert any(x[1] == "step" for x in table[i + 1:i + 5]), (name, i, e)
    # -- E: k grows after it shrank, the order changes, streams and sources alternate, a member is away and returns
    ce = dry["E"]["f"].calls
    ks = [c["k"] for c in ce]
    assert tuple(ks) == E_K
    assert any(a > b and c > b for a, b, c in zip(ks, ks[1:], ks[2:])), ks
    full = [c["members"] for c in ce if c["k"] == 16]
    assert len(full) == 2 and full[0] != full[1] and sorted(full[0]) == sorted(full[1])
    assert sum(a["stream"] != b["stream"] for a, b in zip(ce, ce[1:])) >= 4
    assert {s for c in ce for s in c["sources"]} == {"host", "renderer", "batched"}
    assert all(c["expect"] == (c["k"], 0) for c in ce)
    te = script_e()
    kinds = [e[1:3] for e in te]
    assert ("refuse", "twice") in kinds and ("refuse", "shape") in kinds
    away = [c for c in ce if "e3" not in c["members"]]
    assert ce[2]["k"] == 16 and "e3" not in ce[3]["members"] and "e3" in ce[4]["members"] and len(away) == 3
    assert sum(r["mode"] == "solo" for r in dry["E"]["f"].ses["e3"].records) == 2
    grows = [r for s in dry["E"]["f"].ses.values() for r in s.records if r["mode"] == "B"]
    assert any(-(-r["n_new"] // 256) > -(-r["n"] // 256) for r in grows) and any(-(-r["n_new"] // 256) < -(-r["n"] // 256) for r in grows)
    # -- F: every reason occurs batched and standalone and flips in both directions; the pairs are the rows'
    cf = dry["F"]["f"].calls
    for reason in REASONS:
        seen, flips = set(), set()
        for m in ("big", "u", "g", "c"):
            seq = [c["why"][m][0] for c in cf if m in c["why"] and c["why"][m][1] == reason]
            seen |= set(seq)
            flips |= _flips(seq)
        assert seen == {"B", "S"} and flips == {"BS", "SB"}, (reason, seen, flips)
    for c in cf:
        assert set(c["why"]) == set(c["members"]) and all(c["why"][m][0] == c["modes"][m] for m in c["members"]), c
    assert ("refuse", "cart") in [e[1:3] for e in script_f()]
    rb = dry["F"]["f"].ses["big"].records
    assert {32768, 32769} <= {r["n"] for r in rb} and any(r["n"] == 32769 and r["mode"] == "S" for r in rb)
    ru = dry["F"]["f"].ses["u"].records
    assert [(r["n"], r["mode"]) for r in ru if r["shape"] == WIDE] == [(FORM_N, "S"), (FORM_N - 1, "B"), (FORM_N, "S")]
    # -- G: each listed count is scored and left, in the degenerate members' call among others; every kind of event
    fg = dry["G"]["f"]
    rp = [r for j in range(6) for r in fg.ses[f"p{j}"].records]
    for cnt in COUNTS:
        assert any(r["n"] == cnt for r in rp) and any(r["n"] == cnt and r["n_new"] != cnt for r in rp), cnt
    call = [c for c in fg.calls if "off" in c["members"] and "z" in c["members"] and len(c["members"]) == 9]
    assert len(call) == 1
    in_call = {r["n"] for r in rp if r["call"] == fg.calls.index(call[0])}
    assert in_call == set(COUNTS)
    tg = script_g()
    assert [e[2] for e in tg if e[1] == "map"] == ["maps", "labels", "incremental", "patch"]
    assert {e[3] for e in tg if e[1] == "solo"} == {"freeze", "propagate_freeze0"} and ("init", "i") in [e[1:3] for e in tg]
    assert [e[2] for e in tg if e[1] == "window"] == [(25, 16), (36, 12)]
    assert {e[3] for e in tg if e[1] == "set_states"} == {"equal", "unequal", "offmap"}
    ra = fg.ses["a"].records
    assert {r["ncls"] for r in ra} == {6, 4} and {r["shape"] for r in ra} == {(36, 12), (25, 16)}
    # -- H: the calls of the two fleets alternate; B's staging needs lie below what A left, then A grows past both
    th = [(e[0], e[1], len(e[2])) for e in script_h() if e[1] in ("step", "render", "pose")]
    assert {"A", "B"} == {t[0] for t in th} and sum(a[0] != b[0] for a, b in zip(th, th[1:])) >= 4
    steps = [(t[0], t[2]) for t in th if t[1] == "step"]
    assert steps[:3] == [("A", 3), ("B", 2), ("A", 16)]
    assert dry["H"]["B"].ses["b0"].spec.ncls == 4 and dry["H"]["A"].ses["a0"].spec.ncls == 6


# ---- the sessions on the GPU -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_batch_session_e_membership_and_staging(oracle):
    run(oracle, "E", handle=True)


@pytest.mark.gpu
def test_batch_session_f_eligibility_flips(oracle):
    run(oracle, "F", handle=True)


@pytest.mark.gpu
def test_batch_session_g_state_between_batched_steps(oracle):
    run(oracle, "G", handle=True)


@pytest.mark.gpu
def test_batch_session_h_two_fleets_on_one_thread(oracle):
    run(oracle, "H", handle=True)
