"""Seeded documents over the whole op vocabulary an Automerge 0.12 frontend sends (test input only;
plain Python, no GPU): ``gen_doc(seed)`` returns one document's changes in arrival order, in the
form ``columnar.encode`` takes.

A document is written by a few simulated frontends.  Each has a clock; before a change its author
hears of every other actor with probability GOSSIP and merges that actor's clock.  ``deps`` is the
author's clock minus itself.  An op names only what its author knows: an object or an element whose
creating (actor, seq) is within the author's clock, or which the author made itself.  So every
document is causally valid in generation order, and stays valid however it is delivered.

What the native generators (csrc/synth.cpp) never emit and this one does: counters, incs and
timestamps on any map, table or list element; lists, texts, maps and tables made by any actor at
any time, under map keys and under list elements; table rows; elements inserted and never assigned;
concurrent inserts that collide on ``elem``; several lists and texts in one document.

``fault=`` injects one throwing op (FAULTS names the kinds, one per error status of columnar.STATUS)
into a random change at a random op position; ``gen_doc_info`` also says where it went.
"""
import random

from hypermerge_amd.columnar import ROOT_ID

GOSSIP = 0.35
MAX_OBJECTS = 24
KEYS = ["k0", "k1", "k2", "k3", "k4", "n", "title"]
FAULTS = ("UNKNOWN_OBJECT", "DUPLICATE_OBJECT", "DUPLICATE_ELEM", "MISSING_ELEM", "INCONSISTENT_SEQ")
MAKES = {"map": "makeMap", "table": "makeTable", "list": "makeList", "text": "makeText"}

# (n_actors range, n_changes range)
PROFILES = {
    "default": ((2, 6), (3, 60)),        # documents on both sides of the small kernel's 256-op bound
    "wide": ((9, 40), (20, 60)),         # the general kernel's rows above 8 actors
    "long": ((2, 4), (120, 300)),        # more than 64 changes
}


class _Obj:
    def __init__(self, oid, kind, made_by):
        self.id, self.kind, self.made_by = oid, kind, made_by
        self.keys = []           # map / table: keys somebody assigned (pool keys and row uuids)
        self.elems = []          # list / text: (elemId, elem, made_by)


class _Gen:
    def __init__(self, seed, n_actors, n_changes, fault, profile):
        self.rng = rng = random.Random(seed)
        (a_lo, a_hi), (c_lo, c_hi) = PROFILES[profile]
        na = n_actors if n_actors is not None else rng.randint(a_lo, a_hi)
        self.n_changes = n_changes if n_changes is not None else rng.randint(c_lo, c_hi)
        self.actors = []
        while len(self.actors) < na:                     # random names: rank order differs from index order
            a = f"{rng.getrandbits(32):08x}"
            if a not in self.actors:
                self.actors.append(a)
        self.clock = {a: {} for a in self.actors}
        self.objs = [_Obj(ROOT_ID, "map", None)]
        self.fault = fault
        self.fault_at = rng.randrange(self.n_changes) if fault else -1
        self.info = {}
        self.changes = []

    # -- what the author of the change being written knows
    def knows(self, made_by):
        if made_by is None:
            return True
        a, s = made_by
        return a == self.me or self.clock[self.me].get(a, 0) >= s

    def known_objs(self, kinds):
        return [o for o in self.objs if o.kind in kinds and self.knows(o.made_by)]

    def known_elems(self, o):
        return [e for e in o.elems if self.knows(e[2])]

    def uuid(self):
        r = self.rng
        return f"{r.getrandbits(32):08x}-{r.getrandbits(16):04x}-4{r.getrandbits(12):03x}-8{r.getrandbits(12):03x}-{r.getrandbits(48):012x}"

    def scalar(self):
        r = self.rng
        return r.choice([r.randint(-99, 99), r.randint(0, 999) / 8, r.random(), f"s{r.randrange(40)}", True, False, None,
                         (1 << 32) + r.randrange(1 << 20), (1 << 40) * r.randint(1, 9)])

    def number(self):
        r = self.rng
        return r.choice([r.randint(-9, 9), r.randint(-9, 9), r.randint(-90, 90) / 8, r.random() * 3])

    # -- ops
    def make(self, kind):
        o = _Obj(self.uuid(), kind, self.stamp)
        self.objs.append(o)
        self.ops.append({"action": MAKES[kind], "obj": o.id})
        return o

    def new_kind(self):
        return self.rng.choice(["map", "map", "table", "list", "list", "list", "text"])

    def insert(self, o, after=None):
        """one ``ins`` into list/text o; returns the new element's id"""
        known = self.known_elems(o)
        if after is None:
            after = "_head" if not known or self.rng.random() < 0.25 else self.rng.choice(known)[0]
        elem = max((e[1] for e in known), default=0) + 1       # concurrent authors collide on elem
        eid = f"{self.me}:{elem}"
        self.ops.append({"action": "ins", "obj": o.id, "key": after, "elem": elem})
        o.elems.append((eid, elem, self.stamp))
        return eid

    def element_value(self, o, eid):
        """what follows an insert: a set, a counter set, a link to a new object, or nothing"""
        r = self.rng.random()
        if o.kind == "text":
            if r < 0.85:
                self.ops.append({"action": "set", "obj": o.id, "key": eid, "value": self.rng.choice("abcdefgh ")})
            return
        if r < 0.55:
            self.ops.append({"action": "set", "obj": o.id, "key": eid, "value": self.scalar()})
        elif r < 0.70:
            self.ops.append({"action": "set", "obj": o.id, "key": eid, "value": self.number(), "datatype": "counter"})
        elif r < 0.85 and len(self.objs) < MAX_OBJECTS:
            child = self.make(self.new_kind())
            self.ops.append({"action": "link", "obj": o.id, "key": eid, "value": child.id})
            self.fill(child)
        # else: inserted, never assigned

    def fill(self, o):
        """a new object rarely stays empty"""
        if self.rng.random() < 0.3:
            return
        if o.kind in ("list", "text"):
            after = None
            for _ in range(self.rng.randint(1, 3)):
                after = self.insert(o, after)
                self.ops.append({"action": "set", "obj": o.id, "key": after,
                                 "value": self.rng.choice("xyz") if o.kind == "text" else self.scalar()})
        elif o.kind == "table":
            self.table_row(o)
        else:
            self.map_set(o, self.rng.choice(KEYS))

    def map_set(self, o, key):
        if key not in o.keys:
            o.keys.append(key)
        self.ops.append({"action": "set", "obj": o.id, "key": key, "value": self.scalar()})

    def table_row(self, t):
        key = self.uuid()
        if len(self.objs) >= MAX_OBJECTS:
            return self.map_set(t, key)
        row = self.make("map")
        t.keys.append(key)
        self.ops.append({"action": "link", "obj": t.id, "key": key, "value": row.id})
        for k in self.rng.sample(KEYS, self.rng.randint(0, 2)):
            self.map_set(row, k)

    def map_op(self):
        r = self.rng
        o = r.choice(self.known_objs(("map", "table")))
        key = r.choice(o.keys) if o.keys and (o.kind == "table" or r.random() < 0.3) else r.choice(KEYS)
        x = r.random()
        if x < 0.38:
            self.map_set(o, key)
            if r.random() < 0.10:                                   # the same key twice in one change
                self.map_set(o, key)
        elif x < 0.50:
            self.ops.append({"action": "del", "obj": o.id, "key": key})
        elif x < 0.62:
            if key not in o.keys:
                o.keys.append(key)
            self.ops.append({"action": "set", "obj": o.id, "key": key, "value": self.number(), "datatype": "counter"})
        elif x < 0.80:                                              # on whatever is there
            self.ops.append({"action": "inc", "obj": o.id, "key": key, "value": self.number()})
        elif x < 0.86:
            if key not in o.keys:
                o.keys.append(key)
            self.ops.append({"action": "set", "obj": o.id, "key": key, "value": 1_500_000_000_000 + r.randrange(10 ** 9),
                             "datatype": "timestamp"})
        elif o.kind == "table":
            self.table_row(o)
        else:
            self.create_under_key(o, key)

    def create_under_key(self, o, key):
        if len(self.objs) >= MAX_OBJECTS:
            return self.map_set(o, key)
        if key not in o.keys:
            o.keys.append(key)
        child = self.make(self.new_kind())
        self.ops.append({"action": "link", "obj": o.id, "key": key, "value": child.id})
        self.fill(child)

    def list_op(self):
        r = self.rng
        lists = self.known_objs(("list", "text"))
        if not lists:
            root = self.objs[0]
            return self.create_under_key(root, r.choice(KEYS))
        o = r.choice(lists)
        known = self.known_elems(o)
        x = r.random()
        if x < 0.30 or not known:
            self.element_value(o, self.insert(o))
        elif x < 0.50:                                              # a typed run
            after = None
            for _ in range(r.randint(1, 4)):
                after = self.insert(o, after)
                self.ops.append({"action": "set", "obj": o.id, "key": after,
                                 "value": r.choice("abcdefgh ") if o.kind == "text" else self.scalar()})
        else:
            eid = r.choice(known)[0]
            if x < 0.68:
                self.ops.append({"action": "set", "obj": o.id, "key": eid,
                                 "value": r.choice("abcdefgh ") if o.kind == "text" else self.scalar()})
            elif x < 0.82:
                self.ops.append({"action": "del", "obj": o.id, "key": eid})
            elif x < 0.94:
                self.ops.append({"action": "inc", "obj": o.id, "key": eid, "value": self.number()})
            else:
                self.ops.append({"action": "set", "obj": o.id, "key": eid, "value": self.number(), "datatype": "counter"})

    # -- the injected throwing op
    def fault_ops(self):
        """(ops that set the fault up, the throwing op).  The throwing op names nothing this very
        change makes: it may land in front of that."""
        r, kind = self.rng, self.fault
        older = lambda objs: [o for o in objs if o.made_by != self.stamp]
        if kind == "UNKNOWN_OBJECT":
            return [], {"action": "set", "obj": self.uuid(), "key": "k0", "value": 1}
        if kind == "DUPLICATE_OBJECT":
            cands = [o for o in older(self.known_objs(MAKES)) if o.made_by is not None]
            if cands:
                o = r.choice(cands)
                return [], {"action": MAKES[r.choice(list(MAKES))], "obj": o.id}
            oid = self.uuid()
            return [{"action": "makeMap", "obj": oid}], {"action": "makeList", "obj": oid}
        pre = []
        lists = older(self.known_objs(("list", "text")))
        if lists:
            oid = r.choice(lists).id
            own = [e for o in lists for e in o.elems if e[2][0] == self.me and e[2] != self.stamp]
        else:
            oid, own = self.uuid(), []
            pre = [{"action": "makeList", "obj": oid}, {"action": "link", "obj": ROOT_ID, "key": "faulty", "value": oid}]
        if kind == "MISSING_ELEM":
            return pre, {"action": "set", "obj": oid, "key": f"{self.me}:{9000 + r.randrange(99)}", "value": 1}
        assert kind == "DUPLICATE_ELEM"
        if own:
            e = r.choice(own)
            o = next(o for o in lists if e in o.elems)
            return [], {"action": "ins", "obj": o.id, "key": "_head", "elem": e[1]}
        elem = 8000 + r.randrange(99)
        return pre + [{"action": "ins", "obj": oid, "key": "_head", "elem": elem}], \
            {"action": "ins", "obj": oid, "key": "_head", "elem": elem}

    def inject(self, change):
        """put the throwing op at a random position of the change being written"""
        if self.fault == "INCONSISTENT_SEQ":                    # a second change of this (actor, seq), other content
            twin = dict(change, ops=change["ops"] + [{"action": "set", "obj": ROOT_ID, "key": "twin", "value": 1}])
            self.changes.append(twin)
            self.info = {"kind": self.fault, "actor": change["actor"], "seq": change["seq"], "op": None}
            return
        pre, op = self.fault_ops()
        at = self.rng.randint(0, len(change["ops"]))
        # an op of the change that refers to what the set-up makes cannot come before it: the set-up
        # goes first and the throwing op anywhere behind it
        change["ops"][:0] = pre
        at += len(pre)
        change["ops"].insert(at, op)
        self.info = {"kind": self.fault, "actor": change["actor"], "seq": change["seq"], "op": at}

    def run(self):
        r = self.rng
        for i in range(self.n_changes):
            self.me = me = r.choice(self.actors)
            mine = self.clock[me]
            for other in self.actors:
                if other != me and r.random() < GOSSIP:
                    for a, s in self.clock[other].items():
                        if s > mine.get(a, 0):
                            mine[a] = s
            seq = mine.get(me, 0) + 1
            self.stamp = (me, seq)
            self.ops = []
            for _ in range(r.randint(0, 5)):
                x = r.random()
                if x < 0.45:
                    self.map_op()
                else:
                    self.list_op()
            change = {"actor": me, "seq": seq, "deps": {a: s for a, s in mine.items() if a != me}, "ops": self.ops}
            self.changes.append(change)
            if i == self.fault_at:
                self.inject(change)
            mine[me] = seq
        return self.deliver()

    def deliver(self):
        r, chs = self.rng, self.changes
        x = r.random()
        if x < 0.40:
            r.shuffle(chs)
        elif x < 0.70:
            for _ in range(r.randint(1, 3)):
                chs.insert(r.randint(0, len(chs)), r.choice(chs))
        return chs


def gen_doc_info(seed, n_actors=None, n_changes=None, fault=None, profile="default"):
    """(changes in arrival order, where the injected fault went: kind, actor, seq, op index | None)"""
    assert fault is None or fault in FAULTS
    g = _Gen(seed, n_actors, n_changes, fault, profile)
    return g.run(), g.info


def gen_doc(seed, n_actors=None, n_changes=None, fault=None, profile="default"):
    """One document: a list of Automerge 0.12 change dicts, in arrival order."""
    return gen_doc_info(seed, n_actors, n_changes, fault, profile)[0]


def gen_docs(profile, seeds, **kw):
    return [gen_doc(s, profile=profile, **kw) for s in seeds]


def withheld(chs, seed):
    """(kept, dropped): a delivery that never brings one to three of the document's changes (never
    all of them).  ``kept`` is the arrival list without any copy of the chosen (actor, seq), so every
    change that depends on one of them stays queued; ``dropped`` is one copy of each, sorted by
    (actor, seq): a frontend's changes that have not arrived yet."""
    rng = random.Random(seed)
    names = sorted({(c["actor"], c["seq"]) for c in chs})
    k = min(rng.randint(1, 3), len(names) - 1)
    gone = set(rng.sample(names, k))
    kept = [c for c in chs if (c["actor"], c["seq"]) not in gone]
    first = {}
    for c in chs:
        first.setdefault((c["actor"], c["seq"]), c)
    return kept, [first[n] for n in sorted(gone)]


def base_clock(c):
    """A change as a would-be local change: its base clock by actor id, {...deps}; base[actor] = seq - 1."""
    base = dict(c["deps"])
    base[c["actor"]] = c["seq"] - 1
    return base


def assigned(c):
    """The (obj, key) of a change's set / del / link / inc ops, each once, in op order."""
    out = []
    for op in c["ops"]:
        if op["action"] in ("set", "del", "link", "inc") and (op["obj"], op["key"]) not in out:
            out.append((op["obj"], op["key"]))
    return out


def quiet_tail(chs, k=3):
    """(head, tail): up to k changes that can arrive in a round of their own once everything else
    has been applied, without a new actor, a new object or a change left waiting — what a resident
    store may apply incrementally.  A tail change is the last of its actor (not the actor's first),
    no other change depends on it, and it makes no object; head is the arrival list without any copy
    of the tail changes.  The tail changes are concurrent, so they apply in any order."""
    top, need, first = {}, {}, {}
    for c in chs:
        first.setdefault((c["actor"], c["seq"]), c)
        top[c["actor"]] = max(top.get(c["actor"], 0), c["seq"])
        for a, q in c["deps"].items():
            need[a] = max(need.get(a, 0), q)
    final = [n for n in sorted(first) if n[1] == top[n[0]] and n[1] > 1 and need.get(n[0], 0) < n[1]
             and not any(op["action"] in MAKES.values() for op in first[n]["ops"])]
    tail = set(final[:k])
    return [c for c in chs if (c["actor"], c["seq"]) not in tail], [first[n] for n in sorted(tail)]
