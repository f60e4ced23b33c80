"""Source / destination pairs for the merge-into-a-live-document tests (test input only; plain Python):
hand cases, the wave and tile shapes, and pairs cut from tests/fuzz_docs.py documents.

A case is a dict: src / dst = the two documents' changes in arrival order, clock = {actorId: seq} (its
key order is the hand-over order), have = {actorId: seq} or None (the destination's DocBackend.clock),
order = 'clock' or None (the source's history order)."""
import random

from kat_cases import A, B, Cc, D, ch, d, inc, ins, link, mk, s

Z = "zzzz"


def case(name, src, dst, clock, have=None, order="clock"):
    return {"name": name, "src": src, "dst": dst, "clock": clock, "have": have, "order": order}


SHUFFLED = [ch(B, 2, {A: 2}, s("y", 2)), ch(A, 3, {B: 2}, s("x", 3), s("w", 1)), ch(A, 1, {}, s("x", 1)),
            ch(B, 1, {A: 1}, s("y", 1), d("x")), ch(A, 2, {B: 1}, s("x", 2)), ch(Cc, 1, {A: 3}, s("z", 1))]
TEXT = [ch(A, 1, {}, mk("makeText", "T"), link("t", "T")), ch(A, 2, {}, ins("T", "_head", 1)),
        ch(A, 3, {}, s(f"{A}:1", "h", obj="T")), ch(B, 1, {A: 3}, ins("T", f"{A}:1", 1), s(f"{B}:1", "i", obj="T")),
        ch(A, 4, {B: 1}, d(f"{A}:1", obj="T")), ch(B, 2, {A: 4}, ins("T", "_head", 2), s(f"{B}:2", "!", obj="T"))]
COUNTER = [ch(A, 1, {}, s("n", 10, datatype="counter")), ch(B, 1, {A: 1}, inc("n", 5)), ch(A, 2, {B: 1}, inc("n", -2)),
           ch(B, 2, {A: 2}, s("m", 1.5, datatype="counter")), ch(A, 3, {B: 2}, inc("m", 0.25))]
LINKS = [ch(B, 1, {}, mk("makeMap", "M"), link("m", "M"), s("name", "a string", obj="M")),
         ch(B, 2, {}, mk("makeList", "L"), link("l", "L", obj="M"), ins("L", "_head", 1), s(f"{B}:1", "item", obj="L")),
         ch(Cc, 1, {B: 2}, s("name", "another", obj="M"), s("flag", True))]

HAND = [
    # the reference's "Test document merging": {foo: 'bar'} takes {baz: 'bah'} at {id2: 1}; id2 sorts first
    case("repo_merge", [ch(A, 1, {}, s("baz", "bah"))], [ch(B, 1, {}, s("foo", "bar"))], {A: 1}),
    # the whole shuffled document, actor after actor, into a document with registers and an object of its own
    case("shuffled", SHUFFLED, [ch(Z, 1, {}, s("own", 1), mk("makeMap", "own-map"), link("o", "own-map"), s("k", 2, obj="own-map"))],
         {B: 2, A: 3, Cc: 1}),
    case("shuffled_history_order", SHUFFLED, [ch(D, 1, {}, s("x", 9))], {A: 3, B: 2, Cc: 1}, order=None),
    # a text into a document that holds another text and the source's first two changes: parent renamed,
    # HM_HEAD and elem kept
    case("text", TEXT, [ch(Z, 1, {}, mk("makeText", "U"), link("u", "U"), ins("U", "_head", 1), s(f"{Z}:1", "z", obj="U"))] + TEXT[:2],
         {A: 4, B: 2}),
    # an f64 counter with incs on both sides: dddd's inc is the destination's own
    case("counter", COUNTER, [COUNTER[0], ch(D, 1, {A: 1}, inc("n", 0.5))], {A: 3, B: 2}),
    # links, a nested list, string values
    case("links", LINKS, [ch(A, 1, {}, s("flag", False), mk("makeMap", "N"), link("m", "N"))], {Cc: 1, B: 2}),
    # the destination's queued change (it needs aaaa:3) is unblocked by the merge
    case("unblocks", SHUFFLED, [SHUFFLED[5], ch(Z, 1, {}, s("q", 1))], {A: 3, B: 2}),
    # have below what the destination holds, equal content: the re-handed changes are duplicates (hist -2)
    case("rehanded", SHUFFLED, [SHUFFLED[2], SHUFFLED[3]], {A: 2, B: 2}, have={}),
    # an empty selection: the clock names nothing above what the destination was handed
    case("empty", SHUFFLED, [SHUFFLED[2], SHUFFLED[3], ch(Z, 1, {}, s("q", 1))], {A: 1, B: 1}),
    # a clock that is not causally closed: bbbb's changes wait in the destination's queue
    case("not_closed", SHUFFLED, [ch(Z, 1, {}, s("q", 1))], {B: 2}),
]
HAND_BY_NAME = {c["name"]: c for c in HAND}

# have below what the destination holds, different content: Inconsistent reuse of sequence number
INCONSISTENT = case("inconsistent", SHUFFLED, [ch(A, 1, {}, s("x", 77)), ch(Z, 1, {}, s("q", 1))], {A: 2, B: 1}, have={})


def one_actor_70():
    """One actor with 70 changes and have inside them: the selection crosses the 64-row stride."""
    src = [ch(A, q, {}, s("k%d" % (q % 7), q)) for q in range(1, 71)]
    return case("one_actor_70", src, src[:3] + [ch(B, 1, {}, s("own", 0))], {A: 70})


def two_actors_300():
    """Two actors x 300 changes, have = (10, 0), clock = (300, 290): 580 changes, past the 512-position tile."""
    src = [ch(a, q, {}, s("%s%d" % (a[0], q % 7), q)) for q in range(1, 301) for a in (A, B)]
    dst = [c for c in src if c["actor"] == A and c["seq"] <= 10] + [ch(Cc, 1, {}, s("own", 0))]
    return case("two_actors_300", src, dst, {A: 300, B: 290})


def permuted_maps():
    """70 registers and 70 objects the two documents intern in opposite orders: the object and register
    maps are permutations of more than 64 entries, not the identity."""
    names = ["obj-%02d" % i for i in range(70)]
    src = [ch(A, 1, {}, *[op for i, u in enumerate(names) for op in (mk("makeMap", u), link("l%02d" % i, u), s("v", i, obj=u))])]
    dst = [ch(B, 1, {}, *[op for i, u in reversed(list(enumerate(names))) for op in (mk("makeMap", u + "-b"), link("l%02d" % i, u + "-b"))])]
    # the destination has also heard of the source's objects, in reversed order: a change of cccc that links
    # them waits in its queue (for dddd:9) — never applied, but interned
    dst.append(ch(Cc, 1, {D: 9}, *[link("r%02d" % i, u) for i, u in reversed(list(enumerate(names)))]))
    return case("permuted_maps", src, dst, {A: 1})


def fuzz_pair(chs, seed):
    """A pair cut from one generated document: the source holds all of it; the destination holds a change
    of its own (an actor that sorts last, so every actor it gains re-ranks it), the changes of a random
    half of the actors, and a random prefix of one other actor's; the clock is the source's, cut at random."""
    rng = random.Random(seed)
    actors = sorted({c["actor"] for c in chs})
    mine = set(rng.sample(actors, len(actors) // 2))
    rest = [a for a in actors if a not in mine]
    part = rng.choice(rest)
    upto = rng.randint(0, max(c["seq"] for c in chs if c["actor"] == part))
    own = ch("~" + Z, 1, {}, s("own", seed), mk("makeList", "own-list-%d" % seed), link("ol", "own-list-%d" % seed),
             ins("own-list-%d" % seed, "_head", 1), s("~%s:1" % Z, "e", obj="own-list-%d" % seed))
    dst = [own] + [c for c in chs if c["actor"] in mine or (c["actor"] == part and c["seq"] <= upto)]
    top = {}
    for c in chs:
        top[c["actor"]] = max(top.get(c["actor"], 0), c["seq"])
    keys = list(actors)
    rng.shuffle(keys)
    clock = {a: rng.randint(0, top[a] + 1) for a in keys}
    return case("fuzz_%d" % seed, chs, dst, clock)
