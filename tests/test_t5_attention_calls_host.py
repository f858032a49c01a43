"""The host checks of the six short fused-attention entry points (csrc/t5_attention.hip: rqhip_t5_attention, _fwd_train,
_bwd and their _packed twins), pinned against a recording (tests/golden/t5_attention_call_errors.json).  No GPU needed.

Every case is a call that returns before any device call: a branch of check_att_call or check_packed_call, the
null-pointer and alignment tests, the limit on query rows per K/V group, and the early returns at R = 0 and n_q = 0.
Its (return code, rqhip_last_error() text) is compared with what a library built at the commit before the six entry
points became forwards to three shared calls gave for the same arguments.  No message holds a pointer value.  After a
call that returns 0 the text is the previous call's, so "" is recorded in its place.

Pointers are null or small fake addresses that nothing dereferences: 16 where a check wants an aligned pointer, 8 where it
wants a misaligned one.  A case whose every check passes would launch on them, so each case below ends in a check that
fails or in an early return; the defaults leave q, k, v and out null, which the checks look at last."""
import functools
import json
import os

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "t5_attention_call_errors.json")

A, AT, AB = "rqhip_t5_attention", "rqhip_t5_attention_fwd_train", "rqhip_t5_attention_bwd"
P, PT, PB = "rqhip_t5_attention_packed", "rqhip_t5_attention_packed_fwd_train", "rqhip_t5_attention_packed_bwd"
PADDED, PACKED, TRAIN, ALL = (A, AT, AB), (P, PT, PB), (AT, AB, PT, PB), (A, AT, AB, P, PT, PB)

_FWD, _TRAIN = "bias n_delta offset key_mask causal", "bias n_delta offset key_mask causal p seed"
_BWD_HEAD, _BWD_TAIL = "q ld_q k v ld_kv out ld_out lse d_out ld_do R", _TRAIN + " d_q d_k d_v dtable partial"
ARGS = {A: "q ld_q k v ld_kv R Rk H d_kv Tq Tk " + _FWD + " past anc ld_anc slab_rows out ld_out",
        AT: "q ld_q k v ld_kv R Rk H d_kv Tq Tk " + _TRAIN + " out ld_out lse",
        AB: _BWD_HEAD + " Rk H d_kv Tq Tk " + _BWD_TAIL,
        P: "q ld_q k v ld_kv R n_q n_k H d_kv Tq Tk cu_q cu_k " + _FWD + " out ld_out",
        PT: "q ld_q k v ld_kv R n_q n_k H d_kv Tq Tk cu_q cu_k " + _TRAIN + " out ld_out lse",
        PB: _BWD_HEAD + " n_q n_k H d_kv Tq Tk cu_q cu_k " + _BWD_TAIL}
DEFAULTS = dict(q=None, k=None, v=None, out=None, lse=None, d_out=None, d_q=None, d_k=None, d_v=None, dtable=None,
                partial=None, ld_q=128, ld_kv=128, ld_out=128, ld_do=128, R=4, Rk=4, H=2, d_kv=64, Tq=8, Tk=8, bias=None,
                n_delta=0, offset=0, key_mask=None, causal=0, past=0, anc=None, ld_anc=4, slab_rows=4, p=0.0, seed=None,
                cu_q=16, cu_k=16, n_q=20, n_k=20)       # packed: both tables, 20 of at most R * T = 32 rows a side

Q_SIDE, K_SIDE = ("q", "out", "lse", "d_out", "d_q"), ("k", "v", "d_k", "d_v")


def _ptrs(value, names=Q_SIDE + K_SIDE):
    return {n: value for n in names}


_BIAS = dict(bias=16, n_delta=15, offset=7)             # covers the deltas -7 .. 7 of Tq = Tk = 8
#        case: (entry points, overrides)
CASES = {
    # check_att_call, in its order
    "sizes-H0": (ALL, dict(H=0)),
    "sizes-R-negative": (ALL, dict(R=-1, Rk=-1)),
    "d_kv-32": (ALL, dict(d_kv=32)),
    "Tk-257": (ALL, dict(Tk=257)),
    "Tq-257": (ALL, dict(Tq=257, Tk=256)),
    "one-kv-per-row": ((AT, AB), dict(Rk=2)),
    "not-a-multiple": ((A,), dict(R=10)),
    "no-kv-groups": ((A,), dict(Rk=0)),
    "stride-short": (ALL, dict(ld_kv=124)),
    "stride-odd": (ALL, dict(ld_q=130)),
    "stride-d_out": ((AB, PB), dict(ld_do=126)),
    "ancestor-Tq2": ((A,), dict(anc=16, Tq=2, Tk=3, past=2)),
    "ancestor-Tk": ((A,), dict(anc=16, Tq=1, Tk=5, past=2)),
    "causal-Tq-over-Tk": (ALL, dict(causal=1, Tk=4)),           # packed: check_packed_call's rejection of causal
    "causal-past-over-Tk": ((A,), dict(causal=1, past=2)),
    "bias-Tq-over-Tk": (ALL, dict(bias=16, n_delta=11, offset=7, Tk=4)),
    "bias-table-short": (ALL, dict(_BIAS, n_delta=14)),
    "bias-offset-low": (ALL, dict(_BIAS, offset=6)),
    "p-one": (TRAIN, dict(p=1.0)),
    "p-negative": (TRAIN, dict(p=-0.25)),
    "too-many-workgroups": (ALL, dict(R=2 ** 30, Rk=2 ** 30)),
    # check_packed_call
    "no-table": (PACKED, dict(cu_q=None, cu_k=None)),
    "key-mask": (PACKED, dict(key_mask=16)),
    "n_q-over-R-Tq": (PACKED, dict(n_q=33)),
    "n_k-negative": (PACKED, dict(n_k=-1)),
    "n_k-int32": (PACKED, dict(n_k=2 ** 31)),
    "dense-q-rows": (PACKED, dict(cu_q=None, n_q=20)),
    "dense-k-rows": (PACKED, dict(cu_k=None, n_k=20)),
    # the early returns
    "nothing-to-do": (PADDED, dict(R=0, Rk=0)),
    "nothing-to-do-packed": (PACKED, dict(R=0, n_q=0, n_k=0)),
    "no-queries": ((P, PT), dict(cu_k=None, n_q=0, n_k=32)),
    "no-rows-but-a-bias-table": ((AB,), dict(_BIAS, R=0, Rk=0)),          # goes on to the bias gradient: null pointers
    "no-rows-but-a-bias-table-packed": ((PB,), dict(_BIAS, R=0, n_q=0, n_k=0)),
    # null pointers and alignment
    "null-pointers": (ALL, {}),
    "null-lse": ((AT, PT), _ptrs(16, ("q", "k", "v", "out"))),
    "null-seed": (TRAIN, dict(_ptrs(16), p=0.1)),
    "null-kv": (PACKED, _ptrs(16, Q_SIDE)),
    "null-bias-gradients": ((AB, PB), dict(_ptrs(16), **_BIAS)),
    "misaligned": (ALL, _ptrs(8)),
    "empty-kv-side-may-be-null": (PACKED, dict(_ptrs(8, Q_SIDE), n_k=0)),  # past the null test: the alignment's message
    "empty-q-side-may-be-null": ((PB,), dict(_ptrs(8, K_SIDE), n_q=0)),
    # the inference call's limit on query rows per K/V group
    "beams-limit": ((A,), dict(_ptrs(16), R=2 ** 24, Rk=1, Tq=1)),
}
IDS = [f"{entry}:{case}" for case, (entries, _) in CASES.items() for entry in entries]


def call(l, entry, overrides):
    """One call of `entry` with the defaults and the overrides -> [return code, message or ""]."""
    values = dict(DEFAULTS, **overrides)
    rc = getattr(l, entry)(*[values[name] for name in ARGS[entry].split()], None)
    return [rc, l.rqhip_last_error().decode() if rc != 0 else ""]


def all_results(l):
    """Every case on library `l` -> {case id: [return code, message]}: what the fixture holds."""
    return {f"{entry}:{case}": call(l, entry, over) for case, (entries, over) in CASES.items() for entry in entries}


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)["results"]


def test_the_fixture_holds_every_case_and_nothing_else():
    assert len(IDS) == len(set(IDS)) and sorted(_recorded()) == sorted(IDS)


def test_every_case_returns_what_the_recording_holds():
    from rqhip import _lib
    got, want = all_results(_lib.lib()), _recorded()
    assert {k: v for k, v in got.items() if v != want[k]} == {}
    assert all(rc <= 0 for rc, _ in got.values())       # never a HIP error: no case reached a device call


def test_the_cases_reach_every_message_of_the_checks():
    """Each message of check_att_call, check_packed_call and the calls themselves (by the text behind the entry point's
    name) is recorded for every entry point that can reach it."""
    seen = {entry: set() for entry in ALL}
    for key, (rc, msg) in _recorded().items():
        if rc != 0:
            seen[key.split(":")[0]].add(msg.split(": ", 1)[1])
    everywhere = ("bad sizes", "d_kv=", "Tq=", "the bias table", "null pointer", "q, k, v")     # the last: alignment
    inference = ("R=10 query rows are not", "row strides (q", "the ancestor table", "past + Tq", "Rk * H =",
                 "16777216 query rows")
    one_kv_per_row = ("row strides must be", "Tq = 8 exceeds", "R * H =")     # the training pair and the packed calls
    packed = ("no cumulative table", "a cumulative table goes", "n_q=")
    for entry in ALL:
        want = everywhere + (inference if entry == A else one_kv_per_row)
        want += ("dropout probability",) if entry in TRAIN else ()
        want += ("R=4 query rows over",) if entry in (AT, AB) else ()
        want += packed if entry in PACKED else ()
        for text in want:
            assert any(msg.startswith(text) for msg in seen[entry]), (entry, text)
