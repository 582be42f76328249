"""The compiled reference's answers to tests/test_oracle_vs_reference.py, kept so that those tests run where the
reference cannot be built (TEST INFRASTRUCTURE).

Every call a test makes on the ``reference`` fixture -- its methods, the methods of the sessions it returns and the
oracle_lib helpers that take it as their ``lib`` -- goes through a proxy that makes the same call on a mirror: the
oracle, with sessions of its own that receive the same calls.

* ``RecordingReference`` forwards the call to the real reference and to the mirror.  Where the two answers are equal
  only a running SHA-256 over the call and its answer is kept; where they differ (the reference-only helpers, calls
  whose oracle counterpart deliberately differs) the reference's answer is stored as well.
* ``ReplayReference`` answers from the mirror, or from the stored answer where there is one, and feeds the same
  running digest.  At teardown the number of calls and the digest must equal the recorded ones: a replayed test
  holds the oracle to the reference's answers for exactly the inputs the reference saw.

    PCRAMP_RECORD_REFERENCE=1 python -m pytest tests/test_oracle_vs_reference.py   # rewrites tests/golden/reference_calls.json.gz
"""
import gzip
import hashlib
import json
import os

import numpy as np

TAPE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_calls.json.gz")


def encode(x):
    """A value -> JSON-able form that decode() turns back into an equal value of the same type."""
    if isinstance(x, _SessionProxy):
        return {"s": x._sid}
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, tuple):
        return {"t": [encode(v) for v in x]}
    if isinstance(x, list):
        return [encode(v) for v in x]
    if isinstance(x, dict):
        return {"d": [[k, encode(x[k])] for k in sorted(x)]}
    if isinstance(x, np.ndarray):
        return {"a": x.dtype.str, "shape": list(x.shape), "v": x.ravel().tolist()}
    if isinstance(x, np.generic):
        return {"n": x.dtype.str, "v": x.item()}
    if isinstance(x, bytes):
        return {"b": x.hex()}
    raise TypeError("cannot store %r on the reference tape" % type(x))


def decode(x, sessions=None):
    if isinstance(x, list):
        return [decode(v, sessions) for v in x]
    if not isinstance(x, dict):
        return x
    if "a" in x:
        return np.array(x["v"], dtype=np.dtype(x["a"])).reshape(x["shape"])
    if "s" in x:
        return sessions[x["s"]]
    if "t" in x:
        return tuple(decode(v, sessions) for v in x["t"])
    if "d" in x:
        return {k: decode(v, sessions) for k, v in x["d"]}
    if "n" in x:
        return np.dtype(x["n"]).type(x["v"])
    if "b" in x:
        return bytes.fromhex(x["b"])
    raise ValueError("bad tape value %r" % (x,))


def canonical(x):
    return json.dumps(x, sort_keys=True, separators=(",", ":")).encode()


def load_tapes():
    if not os.path.exists(TAPE_PATH):
        return {}
    with gzip.open(TAPE_PATH, "rt") as f:
        return json.load(f)


def save_tapes(tapes):
    with gzip.GzipFile(TAPE_PATH, "wb", mtime=0) as g:
        g.write(canonical(tapes))


class _SessionProxy:
    def __init__(self, owner, sid):
        self._owner, self._sid = owner, sid

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self._owner._tape_call(self._sid, name, a, k)


def _invoke(lib, sessions, sid, name, args, kwargs, helper):
    """One call on a checker and its sessions -> encoded answer ({"r": ...} or {"raise": ...}) and the raw result."""
    from oracle_lib import Session
    real = [sessions[v._sid] if isinstance(v, _SessionProxy) else v for v in args]
    try:
        if helper is not None:
            res = helper(lib, *real, **kwargs)
        elif sid is None:
            res = getattr(lib, name)(*real, **kwargs)
        else:
            res = getattr(sessions[sid], name)(*real, **kwargs)
    except (RuntimeError, ValueError) as e:
        return {"raise": type(e).__name__, "msg": str(e)}, None
    if isinstance(res, Session):
        sessions.append(res)
        return {"r": {"s": len(sessions) - 1}}, res
    return {"r": encode(res)}, res


class _Proxy:
    def __init__(self, mirror):
        self._mirror, self._mirror_sessions, self._sessions = mirror, [], []
        self._n, self._digest = 0, hashlib.sha256()

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self._tape_call(None, name, a, k)

    def _mirror_call(self, sid, name, args, kwargs, helper):
        if helper is None and sid is None and not hasattr(self._mirror, name):
            return None                                   # a reference-only method
        try:
            return _invoke(self._mirror, self._mirror_sessions, sid, name, args, kwargs, helper)[0]
        except Exception as e:                            # noqa: BLE001  (a signature only the reference has)
            return {"mirror_error": type(e).__name__}

    def _account(self, sid, name, args, kwargs, ans):
        self._digest.update(canonical([self._n, sid, name, encode(tuple(args)), encode(dict(kwargs))]))
        self._digest.update(canonical(ans))
        self._n += 1

    def _answer(self, ans):
        if "raise" in ans:
            raise {"RuntimeError": RuntimeError, "ValueError": ValueError}[ans["raise"]](ans["msg"])
        r = ans["r"]
        if isinstance(r, dict) and set(r) == {"s"}:
            while len(self._sessions) <= r["s"]:
                self._sessions.append(_SessionProxy(self, len(self._sessions)))
        return decode(r, self._sessions)


class RecordingReference(_Proxy):
    """Forwards every call to the real reference (and the mirror) and records the digest and the differing answers."""

    def __init__(self, real, mirror, tape):
        super().__init__(mirror)
        self._real, self._live, self._tape = real, [], tape
        tape.update(calls=0, digest=self._digest.hexdigest(), stored=[])

    def _tape_call(self, sid, name, args, kwargs, helper=None):
        ans, _ = _invoke(self._real, self._live, sid, name, args, kwargs, helper)
        if self._mirror_call(sid, name, args, kwargs, helper) != ans:
            self._tape["stored"].append([self._n, ans])
        self._account(sid, name, args, kwargs, ans)
        self._tape["calls"], self._tape["digest"] = self._n, self._digest.hexdigest()
        return self._answer(ans)


class ReplayReference(_Proxy):
    """Answers every call from the mirror, or from the recorded answer where the reference's differed."""

    def __init__(self, test_id, mirror, tape):
        super().__init__(mirror)
        self._id, self._tape, self._stored = test_id, tape, {i: a for i, a in tape["stored"]}

    def _tape_call(self, sid, name, args, kwargs, helper=None):
        assert self._n < self._tape["calls"], "%s: call %s beyond the %d recorded reference calls" % (self._id, name, self._tape["calls"])
        ans = self._stored.get(self._n)
        mirrored = self._mirror_call(sid, name, args, kwargs, helper)
        if ans is None:
            assert mirrored is not None, "%s: call %d (%s) has no recorded answer" % (self._id, self._n, name)
            ans = mirrored
        self._account(sid, name, args, kwargs, ans)
        return self._answer(ans)

    def _finish(self):
        assert self._n == self._tape["calls"], "%s: %d of %d recorded reference calls made" % (self._id, self._n, self._tape["calls"])
        assert self._digest.hexdigest() == self._tape["digest"], \
            "%s: the oracle's answers (or the calls made) differ from the recorded reference's" % self._id
