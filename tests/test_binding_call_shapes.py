"""The Python binding's call shapes (api.py: _scalar_form_call, _map_form_call, _transforms_call, _map_weights_call, _last_count)
without a device or a built library: a recorder stands in for _lib.lib() and check(), every public method of the weighted, variance,
robust, weighted-robust and map families is driven on a stand-in metric, and per case the C symbol, the argument count, each
argument's kind and the structure of what comes back are held to tests/golden/binding_call_shapes.json.

The fixture is never written from the tree under test: it is this module's records of the binding BEFORE the families were stated
once, `PYTHONPATH=<checkout of that commit> python tests/test_binding_call_shapes.py > tests/golden/binding_call_shapes.json`.
The recorder cannot see how large the buffer behind a pointer is; the GPU tests of every method do."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_call_shapes.json")
N_VIEWS, N_ALPHA, N_T = 4, 5, 6
LOSS, DELTA, FLOOR = 1, 2.5, 0.125


def _kind(a):
    """One argument as the C call gets it, as JSON."""
    if a is None:
        return "None"
    if isinstance(a, C.c_void_p):
        return "c_void_p non-null" if a.value else "c_void_p null"
    if isinstance(a, C.Array):
        return ["array", type(a)._type_.__name__, len(a)]
    if type(a).__name__ == "CArgObject":  # C.byref(x): the letter and the size of x's type
        return ["byref", type(a._obj)._type_, C.sizeof(a._obj)]
    if isinstance(a, bool) or not isinstance(a, (int, float)):
        return ["other", type(a).__name__]
    return [type(a).__name__, a]


def _structure(r):
    """A return value's nesting, and each array's dtype and shape, as JSON."""
    if isinstance(r, (tuple, list)):
        return [type(r).__name__, [_structure(x) for x in r]]
    if isinstance(r, np.ndarray):
        return ["ndarray", str(r.dtype), list(r.shape)]
    if isinstance(r, bool) or not isinstance(r, (int, float)):
        return ["other", type(r).__name__]
    return [type(r).__name__, r]


class _Recorder:
    """Stands in for the loaded library: any ecc_* attribute is a function that records its call and returns 0."""

    def __init__(self):
        self.loads, self.calls = 0, []

    def __getattr__(self, name):
        if not name.startswith("ecc_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append({"symbol": name, "n_args": len(args), "args": [_kind(a) for a in args]})
            return 0
        return fn


class _Dtr:
    def getRadonBinNumber(self, dim):
        return N_T if dim else N_ALPHA


def _metric(api):
    """A metric of N_VIEWS views over 2 * N_VIEWS intermediates that never met a library: what the methods read, nothing else."""
    m = object.__new__(api.MetricRadonIntermediate)
    m.ctx = types.SimpleNamespace(_h=None)
    m._h = C.c_void_p(0x1000)
    m._Ps = np.zeros((N_VIEWS, 12))
    m._dtrs = [_Dtr() for _ in range(2 * N_VIEWS)]
    return m


def _cases():
    """(label, call(metric)) in a fixed order; labels are the fixture's keys."""
    lists = (("empty", np.zeros((0, 4), np.int32)), ("three", [(0, 1, 0, 1), (0, 2, 0, 2), (1, 3, 1, 3)]))
    transforms = (("K0", np.zeros((0, 4, 4))), ("K2", np.stack([np.eye(4), 2.0 * np.eye(4)])))
    forms = (("weighted", ()), ("variance", (FLOOR,)), ("robust", (LOSS, DELTA)), ("weighted_robust", (LOSS, DELTA)))
    out = []
    for want in (False, True):
        w = "pairs" if want else "plain"
        for form, extra in forms:
            out.append(("evaluate_%s/%s" % (form, w),
                        lambda m, f=form, e=extra, want=want: getattr(m, "evaluate_" + f)(*e, want_pairs=want)))
            for how, idx in lists:
                out.append(("evaluate_%s_pairs/%s/%s" % (form, how, w),
                            lambda m, f=form, e=extra, idx=idx, want=want: getattr(m, "evaluate_%s_pairs" % f)(idx, *e, want_pairs=want)))
        for form, extra in (("", ()),) + tuple(("_" + f, e) for f, e in forms):
            for how, Ts in transforms:
                out.append(("evaluate%s_transforms/%s/%s" % (form, how, w),
                            lambda m, f=form, e=extra, Ts=Ts, want=want: getattr(m, "evaluate%s_transforms" % f)(1, Ts, *e, want_pairs=want)))
        for form in ("robust", "weighted_robust"):
            for vname, views in (("all", None), ("two", [2, 0])):
                out.append(("evaluate_%s_map/%s/%s" % (form, vname, w),
                            lambda m, f=form, views=views, want=want: getattr(m, "evaluate_%s_map" % f)(LOSS, DELTA, views=views, want_pairs=want)))
                for how, idx in lists:
                    out.append(("evaluate_%s_map_pairs/%s/%s/%s" % (form, how, vname, w),
                                lambda m, f=form, idx=idx, views=views, want=want:
                                getattr(m, "evaluate_%s_map_pairs" % f)(idx, LOSS, DELTA, views=views, want_pairs=want)))
    for name in ("robust_map_weights", "weighted_robust_map_weights"):
        out.append((name + "/no map", lambda m, name=name: getattr(m, name)()))
        out.append((name + "/after two views",
                    lambda m, name=name: (getattr(m, "evaluate_" + name[:-len("_weights")])(LOSS, DELTA, views=[2, 0]), getattr(m, name)(2.0, 0.5))[1]))
    for name in ("last_evaluated_pairs", "last_batched_poses", "last_gradient_path", "last_batched_transforms"):
        out.append((name, lambda m, name=name: getattr(m, name)()))
    # refused by the binding itself, before the library is touched
    for form, extra in forms:
        out.append(("evaluate_%s_pairs/five indices" % form, lambda m, f=form, e=extra: getattr(m, "evaluate_%s_pairs" % f)([0, 1, 0, 1, 2], *e)))
        out.append(("evaluate_%s_transforms/3x3" % form, lambda m, f=form, e=extra: getattr(m, "evaluate_%s_transforms" % f)(1, np.zeros((3, 3)), *e)))
    out.append(("evaluate_transforms/3x3", lambda m: m.evaluate_transforms(1, np.zeros((3, 3)))))
    for form in ("robust", "weighted_robust"):
        out.append(("evaluate_%s_map/no views" % form, lambda m, f=form: getattr(m, "evaluate_%s_map" % f)(LOSS, DELTA, views=[])))
        out.append(("evaluate_%s_map_pairs/no views" % form, lambda m, f=form: getattr(m, "evaluate_%s_map_pairs" % f)([(0, 1, 0, 1)], LOSS, DELTA, views=[])))
        out.append(("evaluate_%s_map_pairs/five indices" % form, lambda m, f=form: getattr(m, "evaluate_%s_map_pairs" % f)([0, 1, 0, 1, 2], LOSS, DELTA)))
    return out


def record_all(api):
    """Every case on a fresh stand-in metric of `api` (the module epipolarconsistency_amd.api) -> {label: record}."""
    records = {}
    keep = api._lib.lib, api.check
    try:
        for label, call in _cases():
            rec = _Recorder()

            def load(rec=rec):
                rec.loads += 1
                return rec
            api._lib.lib, api.check = load, (lambda code: None)
            m = _metric(api)
            try:
                entry = {"returns": _structure(call(m))}
            except ValueError:
                entry = {"raises": "ValueError", "library_touched": bool(rec.loads)}
            entry["calls"] = rec.calls
            entry["map_count"] = getattr(m, "_robust_map_count", None)
            assert label not in records, label
            records[label] = entry
    finally:
        api._lib.lib, api.check = keep
    return records


def test_call_shapes_are_those_of_the_binding_before_the_drivers():
    from epipolarconsistency_amd import api
    with open(GOLDEN) as f:
        golden = json.load(f)
    got = json.loads(json.dumps(record_all(api)))  # (tuples -> lists, as the fixture has them)
    assert sorted(got) == sorted(golden)
    for label in golden:
        assert got[label] == golden[label], label


def test_fixture_covers_the_families():
    """What the fixture has to hold for the equality above to mean something: every family on both list lengths, both transform
    counts, both view selections, with and without pairs; a refused argument never reaches the library; a committed file's size."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert os.path.getsize(GOLDEN) < (1 << 20)
    assert len(golden) == len(_cases()) == 91
    symbols = {c["symbol"] for e in golden.values() for c in e["calls"]}
    for form in ("weighted", "variance", "robust", "weighted_robust"):
        assert {"ecc_metric_evaluate_" + form, "ecc_metric_evaluate_%s_pairs" % form, "ecc_metric_evaluate_%s_transforms" % form} <= symbols
    assert {"ecc_metric_evaluate_transforms", "ecc_metric_evaluate_robust_map", "ecc_metric_evaluate_robust_map_pairs",
            "ecc_metric_evaluate_weighted_robust_map", "ecc_metric_evaluate_weighted_robust_map_pairs", "ecc_metric_robust_map_weights",
            "ecc_metric_weighted_robust_map_weights", "ecc_metric_last_evaluated_pairs", "ecc_metric_last_batched_poses",
            "ecc_metric_last_gradient_path", "ecc_metric_last_batched_transforms"} <= symbols
    refused = [e for e in golden.values() if "raises" in e]
    assert len(refused) == 15 and all(e["raises"] == "ValueError" and not e["library_touched"] and not e["calls"] for e in refused)


if __name__ == "__main__":  # the fixture, from whichever epipolarconsistency_amd comes first on the path
    from epipolarconsistency_amd import api
    sys.stderr.write("recording %s\n" % api.__file__)
    json.dump(record_all(api), sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
