"""List what a caller of the Python layer can see, one sorted line per item.

usage: python tools/python_surface.py [TREE] > listing.txt

Imports TREE's path-tracer_amd/ (default: this repository) as
`path_tracer_amd`; neither native library has to be built, importing loads
none.  Prints every public name of `path_tracer_amd` and of
`path_tracer_amd.integrator` and, for a class, every public attribute and
method it or a base class of the package defines: each with its kind, its
`inspect.signature` and the first 12 hex digits of the SHA-256 of its
docstring (`-` without one).  A value that is neither a class, a function nor
a module is printed with its repr.  Where an object is defined is not printed,
so that moving it between modules changes nothing; two listings are compared
with `diff`.
"""
from __future__ import annotations

import hashlib
import importlib.util
import inspect
import sys
from pathlib import Path


def load(tree: Path):
    pkg = tree / "path-tracer_amd"
    spec = importlib.util.spec_from_file_location("path_tracer_amd", pkg / "__init__.py",
                                                  submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["path_tracer_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def doc(obj) -> str:
    d = getattr(obj, "__doc__", None)
    return hashlib.sha256(d.encode()).hexdigest()[:12] if isinstance(d, str) else "-"


def sig(obj) -> str:
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return "(?)"


def members(prefix: str, cls: type):
    for name in dir(cls):
        if name.startswith("_"):
            continue
        owner = next(c for c in cls.__mro__ if name in c.__dict__)
        if owner.__module__ == "builtins":
            continue
        m = inspect.getattr_static(cls, name)
        if isinstance(m, property):
            yield f"{prefix}.{name} property{sig(m.fget)} doc={doc(m)}"
        elif isinstance(m, (staticmethod, classmethod)):
            yield f"{prefix}.{name} {type(m).__name__}{sig(m.__func__)} doc={doc(m.__func__)}"
        elif inspect.isfunction(m):
            yield f"{prefix}.{name} method{sig(m)} doc={doc(m)}"
        else:
            yield f"{prefix}.{name} = {m!r}"


def surface(modname: str, mod):
    for name in dir(mod):
        if name.startswith("_"):
            continue
        obj, full = getattr(mod, name), f"{modname}.{name}"
        if inspect.ismodule(obj):
            yield f"{full} module"
        elif inspect.isclass(obj):
            bases = ", ".join(b.__name__ for b in obj.__mro__[1:] if b.__module__ == "builtins" and b is not object)
            yield f"{full} class{sig(obj)} builtin bases=({bases}) doc={doc(obj)}"
            yield from members(full, obj)
        elif inspect.isfunction(obj):
            yield f"{full} function{sig(obj)} doc={doc(obj)}"
        else:
            yield f"{full} = {obj!r}"


def main():
    tree = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).resolve().parent.parent
    pt = load(tree.resolve())
    lines = list(surface("path_tracer_amd", pt)) + list(surface("path_tracer_amd.integrator", pt.integrator))
    print("\n".join(sorted(lines)))


if __name__ == "__main__":
    main()
