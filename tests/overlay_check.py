"""Checks INTEGRATION.md's overlay against the reference tree's interface and the drop-in boundary.

Run by tests/test_overlay.py in a subprocess (it installs stub modules):  python tests/overlay_check.py -> JSON.

The reference tree is not part of this repository.  What the checks need from it -- the names every replaced module defines, the
signatures of its functions and classes, the names its unchanged callers take from the replaced modules, the names the mirrors take
from ``model.networks`` -- is recorded once in tests/golden/overlay_interface.json:
    python tests/overlay_check.py --record [REFERENCE_ROOT]      (the only mode that reads the reference tree)

* overlay: every module listed in 3danimals_amd.overlay.MODULES gets ``overlay.apply(namespace, name)`` on a namespace holding the
  reference module's recorded names -- what the one appended line of INTEGRATION.md does to the module's globals;
* (i)   the imports of the unchanged callers resolve: model.models.{AnimalModel,MagicPony,Fauna,Ponymation}, model.predictors.*,
        model.utils.misc -- every name they import from a replaced module exists after the overlay (the callers are not executed:
        ``imported`` lists those whose imports from the replaced modules all resolve);
* (ii)  every function / class the overlay replaces has a signature that starts with the reference's (same names, order, kinds and
        defaults); anything added must be optional;
* (iii) every attribute the callers take from the replaced modules (mesh.make_mesh, util.perspective, render.render_mesh, ...)
        exists after the overlay, and the hot-path ones are served by this package;
* the mirrors take their networks from ``model.networks`` when that package is importable (a stand-in module with the recorded names).
"""
import ast
import importlib
import importlib.util
import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = "/root/reference"
INTERFACE = os.path.join(HERE, "golden", "overlay_interface.json")
CALLERS = ["model/models/AnimalModel.py", "model/models/MagicPony.py", "model/models/Fauna.py", "model/models/Ponymation.py",
           "model/predictors/BasePredictorBase.py", "model/predictors/BasePredictorBank.py", "model/predictors/InstancePredictorBase.py",
           "model/predictors/InstancePredictorFauna.py", "model/utils/misc.py", "model/render/material.py", "model/render/texture.py",
           "model/render/regularizer.py", "visualization/visualize_results.py"]
IMPORTED_CALLERS = ("model.models.AnimalModel", "model.models.MagicPony", "model.models.Fauna", "model.models.Ponymation",
                    "model.predictors.BasePredictorBase", "model.predictors.BasePredictorBank", "model.predictors.InstancePredictorBase",
                    "model.predictors.InstancePredictorFauna", "model.utils.misc", "model.render.material", "model.render.texture")
NETWORK_NAMES = ("CoordMLP", "CoordMLP_Mod", "MLP")  # what the mirrors import from model.networks when overlaid


def _load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _params(obj):
    """[[name, kind, has_default, repr(default)], ...] of a callable, or None where inspect cannot tell."""
    try:
        sig = inspect.signature(obj)
    except (TypeError, ValueError):
        return None
    return [[p.name, p.kind.name, p.default is not inspect._empty, None if p.default is inspect._empty else repr(p.default)]
            for p in sig.parameters.values()]


def _signature_problems(rp, new_obj, label):
    """The mirror's parameter list must start with the reference's (recorded); extras must be optional."""
    out = []
    if rp is None:
        return out
    try:
        n = inspect.signature(new_obj)
    except (TypeError, ValueError):
        return out
    np_ = list(n.parameters.values())
    for i, (name, kind, has_default, default) in enumerate(rp):
        if kind in ("VAR_POSITIONAL", "VAR_KEYWORD"):
            continue
        if i >= len(np_) or np_[i].name != name or np_[i].kind.name != kind:
            out.append(f"{label}: parameter {i} '{name}' missing or renamed (mirror: {[q.name for q in np_]})")
            break
        b = np_[i].default
        same = (not has_default and b is inspect._empty) or (has_default and b is not inspect._empty and repr(b) == default)
        if not same:
            out.append(f"{label}: default of '{name}' differs (reference {default if has_default else None}, mirror {b!r})")
    ref_names = {p[0] for p in rp}
    for q in np_:
        if q.name not in ref_names and q.default is inspect._empty and q.kind not in (q.VAR_POSITIONAL, q.VAR_KEYWORD):
            out.append(f"{label}: extra parameter '{q.name}' is not optional")
    return out


def record(ref):
    """Read the reference tree once and write tests/golden/overlay_interface.json (names and signatures only)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "3danimals_amd", "shims"), ref]
    mg = _load_make_golden()
    sys.meta_path.insert(0, mg._StubFinder())
    overlay = importlib.import_module("3danimals_amd.overlay")
    rec = dict(modules={}, callers={}, networks=None)
    for name in overlay.MODULES:
        rel = name.replace(".", "/")
        path = os.path.join(ref, rel + ".py") if os.path.exists(os.path.join(ref, rel + ".py")) else os.path.join(ref, rel, "__init__.py")
        mod = importlib.import_module(name)  # the reference module as its callers see it without the overlay
        entry = dict(names=sorted(vars(mod)), callables={})
        for k, old in vars(mod).items():
            if inspect.isclass(old):
                methods = {m: _params(meth) for m, meth in vars(old).items() if (not m.startswith("_") or m == "__call__") and callable(meth)}
                entry["callables"][k] = dict(kind="class", init=_params(old.__init__), methods=methods)
            elif callable(old):
                entry["callables"][k] = dict(kind="function", params=_params(old))
        rec["modules"][name] = entry
        assert os.path.exists(path), path
    networks = importlib.import_module("model.networks")
    rec["networks"] = sorted(n for n in NETWORK_NAMES if hasattr(networks, n))
    for rel in CALLERS:
        path = os.path.join(ref, rel)
        if not os.path.exists(path):
            continue
        tree = ast.parse(open(path).read())
        pkg = os.path.dirname(rel).replace("/", ".")
        alias, uses = {}, []
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom):
                base = node.module or ""
                if node.level:
                    parts = pkg.split(".")
                    parts = parts[: len(parts) - (node.level - 1)]
                    base = ".".join(parts + ([node.module] if node.module else []))
                for a in node.names:
                    full = f"{base}.{a.name}"
                    if full in overlay.MODULES:
                        alias[a.asname or a.name] = full  # from model.render import mesh
                    elif base in overlay.MODULES:
                        uses.append(["from", base, a.name])
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id in alias:
                uses.append(["attr", alias[node.value.id], node.attr])
        rec["callers"][rel] = uses
    with open(INTERFACE, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")


def main():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "3danimals_amd", "shims")]
    rec = json.load(open(INTERFACE))
    # a stand-in for the reference's model.networks, holding the names the mirrors take from it
    pkg = types.ModuleType("model")
    pkg.__path__ = []
    nets = types.ModuleType("model.networks")
    for n in rec["networks"]:
        setattr(nets, n, type(n, (), {}))
    pkg.networks = nets
    sys.modules.update({"model": pkg, "model.networks": nets})
    overlay = importlib.import_module("3danimals_amd.overlay")
    report = dict(imported=[], import_errors={}, signature_problems=[], missing_attributes=[], served_by_reference=[], overlay_applied=[])
    # the overlay on every replaced module: the reference module's recorded globals, then overlay.apply
    modules = {}
    for name in overlay.MODULES:
        try:
            ns = {k: None for k in rec["modules"][name]["names"]}
            modules[name] = overlay.apply(ns, name)
            report["overlay_applied"].append(name)
        except Exception as e:  # noqa: BLE001
            report["import_errors"][name] = f"{type(e).__name__}: {e}"
    report["overlay_applied"] = sorted(report["overlay_applied"])
    # (ii) signatures of what the overlay replaces, against the reference's recorded ones
    for name in overlay.MODULES:
        ref_callables = rec["modules"][name]["callables"]
        for k, new in overlay.exported_names(name).items():
            old = ref_callables.get(k)
            if old is None:
                continue  # an addition of this package (TetGridTopology, SparseBuffers ...)
            if old["kind"] == "class" and inspect.isclass(new):
                report["signature_problems"] += _signature_problems(old["init"], new.__init__, f"{name}.{k}.__init__")
                for mname, rp in old["methods"].items():
                    if not hasattr(new, mname):
                        report["signature_problems"].append(f"{name}.{k}.{mname}: method missing in the mirror")
                    else:
                        report["signature_problems"] += _signature_problems(rp, getattr(new, mname), f"{name}.{k}.{mname}")
            elif old["kind"] == "function":
                report["signature_problems"] += _signature_problems(old["params"], new, f"{name}.{k}")
    # (i) + (iii) what the callers take from the replaced modules
    for rel, uses in rec["callers"].items():
        for how, base, attr in uses:
            if attr not in modules.get(base, {}):
                report["missing_attributes"].append(f"{rel}: {base}.{attr}")
                if how == "from":
                    report["import_errors"][rel[:-3].replace("/", ".")] = f"ImportError: cannot import name '{attr}' from '{base}'"
            elif attr not in overlay.exported_names(base):
                report["served_by_reference"].append(f"{base}.{attr}")
            if how == "from":
                report.setdefault("names_imported", []).append(f"{rel}: from {base} import {attr}")
    report["imported"] = [m for m in IMPORTED_CALLERS if m.replace(".", "/") + ".py" in rec["callers"] and m not in report["import_errors"]]
    report["served_by_reference"] = sorted(set(report["served_by_reference"]))
    report["missing_attributes"] = sorted(set(report["missing_attributes"]))
    dmtet = modules.get("model.geometry.dmtet", {})
    report["networks_in_use"] = getattr(importlib.import_module("3danimals_amd.model.geometry.dmtet"), "NETWORKS", None)
    report["dmtet_overlaid"] = bool(dmtet.get("DMTetGeometry") is not None and dmtet["DMTetGeometry"].__module__.startswith("3danimals_amd"))
    print(json.dumps(report))


if __name__ == "__main__":
    if "--record" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--record"]
        record(rest[0] if rest else REF)
    else:
        main()
