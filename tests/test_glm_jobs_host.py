"""CPU: what the 22 GLM covariance / draw entry points of variance.py hand to the native layer,
call by call and job field by job field, and what the 22 _native wrappers hand to the C
functions, compared with tests/golden/glm_jobs.json.

The golden file is a recording of this module (`python tests/test_glm_jobs_host.py --record`)
made on the commit BEFORE the bindings and the operand parsing were unified; it is never
regenerated with them: a recorded value that has to change is a behaviour change.

Nothing here needs the library or a device: N.require_device is a no-op, the native calls are
recorders that write nothing, the workspace queries return 1000 * nb * (nt or ns or 1) so that a
small max_workspace_bytes forces the runners to chunk.
"""
import ctypes
import inspect
import json
import os
import sys

import pytest
import torch

from conftest import GOLDEN

from bnn_kfac_amd import _native as N
from bnn_kfac_amd import variance as V

GOLDEN_FILE = os.path.join(GOLDEN, "glm_jobs.json")

# native call -> (job struct, the argument after nc: None, "nt" or "ns")
CALLS = {}
for _name, _struct in (("kron_cov", "CovJob"), ("kron_cov_outer", "CovOuterJob"), ("inf_cov", "InfCovJob"),
                       ("inf_cov_outer", "InfCovOuterJob")):
    CALLS[_name] = CALLS[_name + "_tiled"] = (_struct, None)
for _name, _struct in (("kron_cov_sweep", "CovSweepJob"), ("kron_cov_outer_sweep", "CovOuterSweepJob"),
                       ("kron_cov_full", "CovFullJob"), ("kron_cov_outer_full", "CovOuterFullJob")):
    CALLS[_name] = CALLS[_name + "_tiled"] = (_struct, "nt")
CALLS.update(kron_cov_joint=("CovJob", None), kron_cov_outer_joint=("CovOuterJob", None),
             glm_draws=("DrawJob", "ns"), glm_draws_outer=("DrawOuterJob", "ns"),
             inf_draws=("InfDrawJob", "ns"), inf_draws_outer=("InfDrawOuterJob", "ns"))

# variance entry point -> (operand kind, outer?, family)
ENTRIES = {}
for _fn, _kind, _family in (("kron_covariance", "kron", "blocks"), ("kron_covariance_sweep", "sweep", "weighted"),
                            ("kron_covariance_full", "full", "weighted"), ("kron_covariance_inf", "inf", "blocks")):
    _outer = _fn.replace("kron_covariance", "kron_covariance_outer")
    for _suffix in ("", "_tiled"):
        ENTRIES[_fn + _suffix] = (_kind, False, _family)
        ENTRIES[_outer + _suffix] = (_kind, True, _family)
ENTRIES.update(kron_covariance_joint=("kron", False, "joint"), kron_covariance_outer_joint=("kron", True, "joint"),
               kron_draws=("kron", False, "draws"), kron_draws_outer=("kron", True, "draws"),
               kron_draws_inf=("infdraw", False, "draws"), kron_draws_outer_inf=("infdraw", True, "draws"))
assert len(CALLS) == 22 and len(ENTRIES) == 22


def _fields(struct):
    """Flat field names of a ctypes struct, a nested struct's as `rows.J`."""
    out = []
    for name, typ in struct._fields_:
        if issubclass(typ, ctypes.Structure):
            out.extend(f"{name}.{f}" for f in _fields(typ))
        else:
            out.append(name)
    return out


class Recorder:
    """The inputs of one case by name, and the native calls made on them."""

    def __init__(self):
        self.inputs, self.calls = {}, []

    def tensor(self, name, *shape):
        t = self.inputs[name] = torch.zeros(*shape, dtype=torch.float32)
        return t

    def padded(self, name, *shape):
        """(..., n) whose rows lie n + 3 apart; offsets are recorded against the whole buffer."""
        return self.tensor(name, *shape[:-1], shape[-1] + 3)[..., :shape[-1]]

    def locate(self, p):
        """[input name, byte offset] of a pointer into one of the inputs, else "copy"."""
        if not p:
            return None
        for name, t in self.inputs.items():
            extent = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
            if t.data_ptr() <= p < t.data_ptr() + 4 * extent:
                return [name, p - t.data_ptr()]
        return "copy"

    def values(self, job):
        out = []
        for name, typ in job._fields_:
            v = getattr(job, name)
            if issubclass(typ, ctypes.Structure):
                out.extend(self.values(v))
            else:
                out.append(self.locate(v) if typ is ctypes.c_void_p else v)
        return out

    def stub(self, name):
        struct, extra = CALLS[name]

        def workspace_bytes(jobs, nb, nc, n=None):
            assert all(type(j) is getattr(N, struct) for j in jobs)
            return 1000 * nb * (n or 1)

        def call(jobs, nb, nc, *rest, accumulate=False):
            n, out = rest if extra else (None, rest[0])
            assert all(type(j) is getattr(N, struct) for j in jobs)
            self.calls.append({"call": name, "nb": nb, "nc": nc, extra or "n": n, "accumulate": bool(accumulate),
                               "out": out, "jobs": [self.values(j) for j in jobs]})

        return workspace_bytes, call

    def finish(self, result):
        """The calls with `out` as (shape, strides, byte offset into the result or "fresh")."""
        for c in self.calls:
            out = c["out"]
            inside = out.untyped_storage().data_ptr() == result.untyped_storage().data_ptr()
            c["out"] = [list(out.shape), list(out.stride()), out.data_ptr() - result.data_ptr() if inside else "fresh"]
        return self.calls


def _operands(rec, l, kind, outer, nb, nc, nt, ns, style):
    """(term l of `kind`, its z, its e) in one of the styles plain / flat (nb = 1: 1-D a, 2-D J
    and D, 1-D or 2-D weights) / padded (row strides used in place) / copied (transposed or
    column-strided: the builders copy) / noones (nA = cols: no implicit ones column)."""
    cols, nG = 2 + l % 3, 2 + l % 2
    nA = cols + (style != "noones")
    ra, rg = 2, 1 + l % 2
    r = ra * rg

    def mat(name, rows, width):
        if style == "padded":
            return rec.padded(f"{l}.{name}", rows, width)
        if style == "copied":
            return rec.tensor(f"{l}.{name}", rows, 2 * width)[:, ::2]
        return rec.tensor(f"{l}.{name}", rows, width)

    def rows3(name, width):
        if style == "flat":
            return rec.tensor(f"{l}.{name}", nc, width)
        return (rec.padded if style == "padded" else rec.tensor)(f"{l}.{name}", nb, nc, width)

    if outer:
        a = (rec.tensor(f"{l}.a", cols) if style == "flat" else rec.tensor(f"{l}.a", cols, nb).t()
             if style == "copied" else mat("a", nb, cols))
        head = (a, rows3("D", nG))
    else:
        head = (rows3("J", nA * nG),)

    def weights(name, n):
        if style == "flat":
            return rec.tensor(f"{l}.{name}", n)
        return rec.tensor(f"{l}.{name}", n, nt).t() if style == "copied" else mat(name, nt, n)

    if kind == "kron":
        tail = (mat("K1", nA, nA), mat("K2", nG, nG))
    elif kind == "sweep":
        tail = (mat("VA", nA, nA), mat("VG", nG, nG), weights("wA", nA), weights("wG", nG))
    elif kind == "full":
        W = (rec.tensor(f"{l}.W", nA, nG) if style == "flat" else rec.tensor(f"{l}.W", nt, nA + 1, nG)[:, :nA]
             if style == "padded" else rec.tensor(f"{l}.W", nt, nG, nA).transpose(1, 2) if style == "copied"
             else rec.tensor(f"{l}.W", nt, nA, nG))
        tail = (mat("VA", nA, nA), mat("VG", nG, nG), W)
    else:
        W = rec.tensor(f"{l}.W", nG, nA).t() if style == "copied" else rec.tensor(f"{l}.W", nA, nG)
        tail = (mat("UA", nA, ra), mat("UG", nG, rg), W, mat("F", r, r))
        if kind == "infdraw":
            tail += (rec.tensor(f"{l}.C", nA, nG), mat("Binv", r, r))
    z = e = None
    if ns:
        if style == "padded":
            z = rec.tensor(f"{l}.z", ns, nA * nG + 2).as_strided((ns, nA, nG), (nA * nG + 2, nG, 1))
        elif style == "copied":
            z = rec.tensor(f"{l}.z", ns, nG, nA).transpose(1, 2)
        else:
            z = rec.tensor(f"{l}.z", ns, nA, nG)
        e = mat("e", ns, r)
    return head + tail, z, e


def _cases(entry):
    """{case: (styles per term, nb, nc, nt, ns, lower, max_workspace_bytes)} of one entry point."""
    kind, outer, family = ENTRIES[entry]
    weighted, draws = family == "weighted", family == "draws"
    nine = ["padded", "copied", "noones"] + ["plain"] * 6
    big = 1 << 30
    cases = {
        "one": (["flat"], 1, 2, 1, 2, False, big),
        # 9 terms fold 8 + 1; 5 samples under the cap go 2 + 2 + 1 (draws: 5 draws go 3 + 2);
        # 65 grid points are two calls; the joint calls cannot be cut
        "nine": (nine, 5, 3, 65 if weighted else 1, 5, True,
                 big if family == "joint" else 2500 * 64 if weighted else 15000 if draws else 2500),
        "none": ([], 0, 0, 0, 0, True, big),
    }
    if draws:  # the draws cut to single ones, then the samples 3 + 2
        cases["cut"] = (["padded", "plain"], 5, 3, 1, 5, True, 3000)
    elif family != "joint":
        tiled = entry.endswith("_tiled")
        cases["wide"] = (["plain"], 2, 33 if tiled else 32, 2, 0, True, big)
        if not tiled:
            cases["over"] = (["plain"], 2, 33, 2, 0, True, big)
    return cases


def _run(entry, styles, nb, nc, nt, ns, lower, cap):
    kind, outer, family = ENTRIES[entry]
    rec = Recorder()
    parts = [_operands(rec, l, kind, outer, nb, nc, nt, ns if family == "draws" else 0, style)
             for l, style in enumerate(styles)]
    terms = [p[0] for p in parts]
    args = [terms]
    if family == "draws":
        args.append([p[1] for p in parts])
        if kind == "infdraw":
            args.append([p[2] for p in parts])
    kwargs = {"max_workspace_bytes": cap}
    if kind == "kron":
        kwargs["lower"] = lower
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(N, "require_device", lambda t, what, owner=None: None)
        for name in CALLS:
            workspace_bytes, call = rec.stub(name)
            mp.setattr(N, name + "_workspace_bytes", workspace_bytes)
            mp.setattr(N, name, call)
        try:
            result = getattr(V, entry)(*args, **kwargs)
        except (ValueError, TypeError, N.NativeError) as err:
            return {"error": [type(err).__name__, str(err)]}
    return {"result": [list(result.shape), list(result.stride())], "calls": rec.finish(result)}


def record_jobs():
    return {f"{entry}/{case}": _run(entry, *spec) for entry in ENTRIES for case, spec in _cases(entry).items()}


# ------------------------------------------------------------------ the _native wrappers
class _Lib:
    """Stands in for N.lib(): every symbol records its positional arguments."""

    def __init__(self, log, describe):
        self._log, self._describe = log, describe

    def __getattr__(self, symbol):
        def fn(*args):
            self._log.append([symbol, [self._describe(a) for a in args]])
            return 5000 if symbol.endswith("_workspace_bytes") else 0
        return fn


class _Workspace:
    def __init__(self, log):
        self._log, self.bufs = log, []

    def get(self, device, nbytes, stream=None, stream_obj=None):
        self._log.append(["workspace.get", [str(device), nbytes]])
        self.bufs.append(torch.zeros(nbytes + 8, dtype=torch.uint8))
        return self.bufs[-1]


def _wrapper(name):
    """What wrapper `name` and its query pass on for 3 samples, 2 outputs and nt / ns = 4: a
    plain call, one with accumulate=True, and for the draw calls one draw into a row whose
    stride is below its width."""
    struct, extra = CALLS[name]
    nb, nc, n = 3, 2, 4
    R = nb * nc
    if extra == "ns":
        outs = [(n, torch.zeros(n, R + 3)[:, :R]), (1, torch.zeros(R).as_strided((1, R), (1, 1)))]
    elif extra == "nt":
        outs = [(n, torch.zeros(n, nb, nc, nc))]
    elif name.endswith("_joint"):
        outs = [(None, torch.zeros(R, R + 3)[:, :R])]
    else:
        outs = [(None, torch.zeros(nb, nc, nc))]
    log = []
    ws = _Workspace(log)

    def describe(a):
        if isinstance(a, ctypes.Array):
            return ["array", a._type_.__name__, len(a)]
        for what, t in [("out", o) for _, o in outs] + [("ws", b) for b in ws.bufs]:
            if a == t.data_ptr():
                return what
        return a

    fn, query = getattr(N, name), getattr(N, name + "_workspace_bytes")
    jobs = [getattr(N, struct)(), getattr(N, struct)()]
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(N, "require_device", lambda t, what, owner=None: None)
        mp.setattr(N, "lib", lambda: _Lib(log, describe))
        mp.setattr(N, "workspace", ws)
        mp.setattr(N, "stream_handle", lambda device: 77)
        for count, out in outs:
            sizes = (nb, nc) if count is None else (nb, nc, count)
            log.append(["query", query(jobs, *sizes)])
            fn(jobs, *sizes, out)
            fn(jobs, *sizes, out, accumulate=True)
    params = [[[p.name, p.kind.name, None if p.default is p.empty else repr(p.default)]
               for p in inspect.signature(f).parameters.values()] for f in (fn, query)]
    return {"log": log, "parameters": params, "doc": fn.__doc__}


def record():
    return json.loads(json.dumps({"fields": {s: _fields(getattr(N, s)) for s, _ in CALLS.values()},
                                  "jobs": record_jobs(), "wrappers": {name: _wrapper(name) for name in CALLS}}))


def _write(path):
    rec = record()
    dump = lambda v: json.dumps(v, separators=(",", ":"), sort_keys=True)  # noqa: E731
    with open(path, "w") as f:
        f.write("{\n")
        for section in ("fields", "jobs", "wrappers"):
            f.write(f'"{section}":{{\n')
            f.write(",\n".join(f"{json.dumps(k)}:{dump(v)}" for k, v in rec[section].items()))
            f.write("\n}" + ("\n" if section == "wrappers" else ",\n"))
        f.write("}\n")


@pytest.fixture(scope="module")
def recorded():
    return record()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_job_struct_fields(recorded, golden):
    assert recorded["fields"] == golden["fields"]


def test_every_case_is_recorded(recorded, golden):
    assert sorted(recorded["jobs"]) == sorted(golden["jobs"])
    assert len(golden["jobs"]) == sum(len(_cases(entry)) for entry in ENTRIES)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_native_calls_match_recording(recorded, golden, entry):
    for case in _cases(entry):
        got, want = recorded["jobs"][f"{entry}/{case}"], golden["jobs"][f"{entry}/{case}"]
        assert ("error" in want) == (case in ("none", "over")), case
        assert got == want, case


def test_recording_reaches_the_branches(golden):
    """The golden file holds what the cases were chosen for."""
    jobs = golden["jobs"]
    calls = jobs["kron_covariance/nine"]["calls"]
    assert len(calls) == 6 and [len(c["jobs"]) for c in calls] == [8, 1] * 3
    assert [c["nb"] for c in calls] == [2, 2, 2, 2, 1, 1] and [c["accumulate"] for c in calls] == [False, True] * 3
    sweep = jobs["kron_covariance_outer_sweep/nine"]["calls"]
    assert sorted({c["nt"] for c in sweep}) == [1, 64] and {c["out"][2] for c in sweep} == {"fresh"}
    draws = jobs["kron_draws_inf/nine"]["calls"]
    assert [c["ns"] for c in draws] == [3, 3, 2, 2] and {c["nb"] for c in draws} == {5}
    cut = jobs["kron_draws_outer/cut"]["calls"]
    assert {c["ns"] for c in cut} == {1} and [c["nb"] for c in cut] == [3] * 5 + [2] * 5
    flat = [v for c in jobs["kron_covariance_outer/nine"]["calls"] for j in c["jobs"] for v in j]
    assert "copy" in flat and any(isinstance(v, list) and v[1] > 0 for v in flat)
    assert jobs["kron_covariance_inf/over"]["error"][1] == "kron_covariance_inf handles at most 32 outputs, got 33"
    assert jobs["kron_covariance_inf_tiled/wide"]["calls"][0]["nc"] == 33


@pytest.mark.parametrize("name", sorted(CALLS))
def test_wrapper_passes_on_what_it_did(recorded, golden, name):
    got, want = recorded["wrappers"][name], golden["wrappers"][name]
    assert got["log"] == want["log"]
    assert got["parameters"] == want["parameters"]
    if want["doc"] is not None:  # (the four class-tiled weighted calls had none)
        assert got["doc"] == want["doc"]
    struct, extra = CALLS[name]
    calls = [args for symbol, args in got["log"] if symbol == "kfac_" + name]
    assert len(calls) in (2, 4) and all(args[0] == ["array", struct, 2] and args[-1] == 77 for args in calls)


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: test_glm_jobs_host.py --record [file]   (on the commit the recording is to pin)")
    _write(sys.argv[2] if len(sys.argv) > 2 else GOLDEN_FILE)
