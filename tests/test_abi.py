"""CPU: the C-ABI library loads and exports every symbol include/geoadv.h declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "geoadv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(geoadv_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    names = _declared()
    for must in ["geoadv_nn_distance", "geoadv_nn_distance_grad", "geoadv_approx_match", "geoadv_match_cost",
                 "geoadv_match_cost_grad", "geoadv_selection_sort", "geoadv_group_point", "geoadv_group_point_grad",
                 "geoadv_query_ball_point", "geoadv_knn_point", "geoadv_attack_run", "geoadv_debug_chamfer_sym_plan"]:
        assert must in names


def test_library_exports_every_declared_symbol():
    import torch  # noqa: F401  -- before the library, so that both bind to one HIP runtime if GPU tests share the process
    from geometric_adv_amd import _lib
    import __graft_entry__
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, "libgeoadv.so lacks: %s" % missing
    assert lib.geoadv_version() >= 1


def _struct_fields(name):
    """(C type, field) pairs of `typedef struct <name> { ... } <name>;` in include/geoadv.h, comments stripped."""
    text = open(os.path.join(ROOT, "include", "geoadv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), text, flags=re.S).group(1)
    return [(t, f) for t, f in re.findall(r"\b(int|float)\s+([a-z0-9_]+)\s*;", body)]


def test_python_mirror_of_the_attack_config_matches_the_header():
    """The ctypes structure adv_ae.py passes to geoadv_attack_create has the header's fields, in order, with the header's types:
    a field added on one side only would shift every later one silently."""
    from geometric_adv_amd.adv_ae import _AttackConfig
    want = _struct_fields("geoadv_attack_config")
    got = [({ctypes.c_int: "int", ctypes.c_float: "float"}[t], f) for f, t in _AttackConfig._fields_]
    assert got == want
    assert want[-1] == ("int", "loss_in_scan")


def test_python_mirror_of_the_train_config_matches_the_header():
    from geometric_adv_amd.trainer import _TrainConfig
    want = _struct_fields("geoadv_train_config")
    got = [({ctypes.c_int: "int", ctypes.c_float: "float"}[t], f) for f, t in _TrainConfig._fields_]
    assert got == want


# ---- include/geoadv.h against geometric_adv_amd/_abi.py: every declaration of the boundary is written once on each side ----------

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char *": ctypes.c_char_p, "void": None}
_HEADER = {}


def _header():
    """include/geoadv.h parsed once: text (comments and preprocessor lines stripped), constants (#define and enum values),
    prototypes {name: (C return type, [C parameter declarations])} in order, structs {name: [C member declarations]}."""
    if _HEADER:
        return _HEADER
    raw = open(os.path.join(ROOT, "include", "geoadv.h")).read()
    raw = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    raw = re.sub(r"//[^\n]*", " ", raw)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(GEOADV_[A-Z0-9_]+)[ \t]+(\S[^\n]*)$", raw, flags=re.M):
        consts[name] = int(eval(value, {"__builtins__": {}}, dict(consts)))
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", raw, flags=re.M)
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, flags=re.S):
        nxt = 0
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, _, value = (x.strip() for x in item.partition("="))
            nxt = int(eval(value, {"__builtins__": {}}, dict(consts))) if value else nxt
            consts[name] = nxt
            nxt += 1
    structs = {}
    for name, body in re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        structs[name] = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    flat = re.sub(r"\{[^{}]*\}", " ", re.sub(r'extern\s+"C"\s*\{', " ", text))      # struct and enum bodies out of the way
    protos = {}
    for stmt in flat.split(";"):
        m = re.match(r"^\s*([A-Za-z_][\w\s\*]*?)\s*\b(geoadv_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if m and not m.group(1).startswith("typedef"):
            assert m.group(2) not in protos, m.group(2)
            params = [" ".join(a.split()) for a in m.group(3).split(",")]
            protos[m.group(2)] = (" ".join(m.group(1).split()), [] if params == ["void"] else params)
    _HEADER.update(text=text, consts=consts, structs=structs, protos=protos)
    return _HEADER


def _param_ctype(decl):
    """The issue's mapping rule for one parameter declaration: every pointer or array is c_void_p, a scalar its own ctypes type."""
    if "*" in decl or "[" in decl:
        return ctypes.c_void_p
    ctype = re.sub(r"\bconst\b", "", decl).split()[:-1]              # the last word is the parameter's name
    return _SCALARS[" ".join(ctype)]


def _member_fields(decl, consts):
    """(name, ctypes type) of every declarator of one struct member declaration, e.g. `const float *enc_w[5], *enc_b[5]`."""
    m = re.match(r"^(?:const\s+)?(unsigned long long|long long|int|float|double|size_t)\s+(.*)$", decl)
    assert m, decl
    out = []
    for d in m.group(2).split(","):
        star, name, dim = re.match(r"^\s*(\*?)\s*([A-Za-z_]\w*)\s*(?:\[(.*)\])?\s*$", d).groups()
        t = ctypes.c_void_p if star else _SCALARS[m.group(1)]
        out.append((name, t * int(eval(dim, {"__builtins__": {}}, dict(consts))) if dim else t))
    return out


def _same_ctype(a, b):
    if hasattr(a, "_length_") or hasattr(b, "_length_"):
        return getattr(a, "_length_", None) == getattr(b, "_length_", None) and a._type_ is b._type_
    return a is b


def test_prototypes_match_the_typed_table():
    from geometric_adv_amd import _abi
    protos = _header()["protos"]
    assert sorted(protos) == _declared()                          # the parser drops no prototype
    assert set(_abi.SIGNATURES) - set(protos) == set() and set(protos) - set(_abi.SIGNATURES) == set()
    assert list(_abi.SIGNATURES) == list(protos)                  # and the table keeps the header's order
    for name, (ret, params) in protos.items():
        restype, argtypes = _abi.ctypes_signature(name)
        assert restype is _RETURNS[ret], name
        assert list(argtypes) == [_param_ctype(p) for p in params], name


def test_loaded_library_carries_the_table():
    import torch  # noqa: F401
    from geometric_adv_amd import _abi, _lib
    import __graft_entry__
    if not os.path.exists(_lib.LIB_PATH):
        __graft_entry__.build()
    lib = _lib.lib()
    assert len(_abi.SIGNATURES) == len(_declared())
    for name in _abi.SIGNATURES:
        restype, argtypes = _abi.ctypes_signature(name)
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == list(argtypes), name


def test_every_struct_of_the_header_has_its_mirror():
    from geometric_adv_amd import _abi
    h = _header()
    assert len(h["structs"]) == 12
    assert set(_abi.STRUCTS) == set(h["structs"])
    for name, members in h["structs"].items():
        want = [f for decl in members for f in _member_fields(decl, h["consts"])]
        got = list(_abi.STRUCTS[name]._fields_)
        assert [f for f, _ in got] == [f for f, _ in want], name
        for (f, a), (_, b) in zip(got, want):
            assert _same_ctype(a, b), (name, f)
    # the cases the parser must not lose: arrays sized by an expression, several declarators on one line, 64-bit members
    ae = dict(_abi.STRUCTS["geoadv_ae_weights"]._fields_)
    assert ae["enc_dims"]._length_ == 6 and ae["enc_dims"]._type_ is ctypes.c_int
    assert ae["enc_b"]._length_ == 5 and ae["enc_b"]._type_ is ctypes.c_void_p
    aug = dict(_abi.STRUCTS["geoadv_batch_augment"]._fields_)
    assert aug["seed"] is ctypes.c_ulonglong and aug["counter"] is ctypes.c_ulonglong
    assert dict(_abi.STRUCTS["geoadv_fold_train_config"]._fields_)["initial_ordinal"] is ctypes.c_longlong


def test_constants_are_the_headers():
    from geometric_adv_amd import _abi, adv_ae, atlas_trainer, autoencoder, cls_trainer, fold_trainer, foldingnet, ops, trainer
    consts = _header()["consts"]
    mine = {k: v for k, v in vars(_abi).items() if k.startswith("GEOADV_")}
    assert len(mine) > 40
    for name, value in mine.items():
        assert name in consts and consts[name] == value, name

    def codes(prefix):
        return {v for k, v in mine.items() if k.startswith(prefix)}
    for table, prefix in [(cls_trainer._STATE, "GEOADV_CLS_STATE_"), (fold_trainer._STATE, "GEOADV_FOLD_STATE_"),
                          (atlas_trainer._STATE, "GEOADV_ATLAS_STATE_"), (trainer.PointNetAETrainer._STATE, "GEOADV_TRAIN_STATE_"),
                          (cls_trainer.OPTIMIZERS, "GEOADV_CLS_OPT_"), (ops.KNN_KERNELS, "GEOADV_KNN_"), (ops.FPS_FORMS, "GEOADV_FPS_"),
                          (ops.NORMALIZATIONS, "GEOADV_NORMALIZE_"), (autoencoder.ENCODER_ARITH, "GEOADV_ENC_ARITH_"),
                          (adv_ae.CHAMFER_KERNELS, "GEOADV_CHAMFER_"), (adv_ae.ENCODER_BACKWARDS, "GEOADV_ENC_BWD_")]:
        assert table and set(table.values()) <= codes(prefix), prefix
        assert len(set(table.values())) == len(table), prefix
    assert len(adv_ae.PROF_NAMES) == _abi.GEOADV_PROF_COUNT
    assert [consts["GEOADV_PROF_" + n.upper()] for n in adv_ae.PROF_NAMES] == list(range(_abi.GEOADV_PROF_COUNT))
    assert ops.EMD_DENSE_LEVELS == consts["GEOADV_EMD_DENSE_LEVELS"] and ops.AUGMENT_RECORD == consts["GEOADV_AUGMENT_RECORD"]
    assert (foldingnet.PICKS_GIVEN, foldingnet.PICKS_DEVICE) == (consts["GEOADV_FOLD_PICKS_GIVEN"], consts["GEOADV_FOLD_PICKS_DEVICE"])
    assert atlas_trainer.MAX_TRAIN_LAYERS == consts["GEOADV_ATLAS_ENC_LAYERS"] + consts["GEOADV_ATLAS_MAX_DEC_LAYERS"]


def test_call_sites_pass_as_many_arguments_as_the_table_has():
    """Every <expr>.geoadv_<name>(...) of the package passes the table's number of positional arguments, every
    _call("geoadv_<name>", ...) one fewer (ops._call appends the stream).  Only the two indirections themselves are not counted:
    the body of ops._call and _model's getattr(lib, self._destroy)(handle), neither of which names its function."""
    import ast
    import glob
    from geometric_adv_amd import _abi
    seen, bad = 0, []
    for path in sorted(glob.glob(os.path.join(ROOT, "geometric_adv_amd", "*.py"))):
        tree = ast.parse(open(path).read(), path)
        skipped = set()
        for node in ast.walk(tree):
            if isinstance(node, ast.FunctionDef) and node.name == "_call" and path.endswith("ops.py"):
                skipped |= set(map(id, ast.walk(node)))
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call) or id(node) in skipped:
                continue
            name = given = None
            if isinstance(node.func, ast.Attribute) and node.func.attr.startswith("geoadv_"):
                name, given = node.func.attr, len(node.args)
            elif isinstance(node.func, ast.Name) and node.func.id == "_call":
                assert isinstance(node.args[0], ast.Constant), "%s:%d" % (path, node.lineno)
                name, given = node.args[0].value, len(node.args)      # the name takes the place of the stream
            if name is None:
                continue
            assert not node.keywords and not any(isinstance(a, ast.Starred) for a in node.args), "%s:%d" % (path, node.lineno)
            seen += 1
            if given != len(_abi.SIGNATURES[name].partition(":")[2]):
                bad.append("%s:%d %s passes %d" % (os.path.basename(path), node.lineno, name, given))
    assert seen >= 90, seen
    assert not bad, bad
