"""CPU tier: the layering of the post-processing Python.  selection.py says which rows and sets,
_device.py gets them to the device, posterior / datafits / moho build on both; every name has one home and no private
name crosses a module boundary.  The package's sources are parsed with ast: neither torch nor a GPU is needed."""
import ast
import importlib
import os

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, 'bayhunter_amd')
TREES = {f[:-3]: ast.parse(open(os.path.join(PKG, f)).read()) for f in sorted(os.listdir(PKG)) if f.endswith('.py')}
SELECTION = ('pool_selection', 'chain_like_medians', 'pool_outliers', 'pool_rows', 'station_rows', 'check_set_start',
             'raise_first_failed', 'SetList', 'StationResult')
DEVICE = ('Handle', 'torch_device', 'to_device', 'device_rows')
STATISTICS = ('posterior', 'datafits', 'moho')


def _defined(tree):
    """Names a module binds at its top level by def, class or assignment."""
    names = set()
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            names.add(node.name)
        elif isinstance(node, ast.Assign):
            names.update(t.id for t in node.targets if isinstance(t, ast.Name))
    return names


def test_the_package_is_there():
    assert len(TREES) > 15 and {'selection', '_device', '_lib'} | set(STATISTICS) <= set(TREES)


def test_no_private_name_crosses_a_module_boundary():
    """`from .X import _name` occurs nowhere in the package (the modules _lib and _device themselves may be imported)."""
    for mod, tree in TREES.items():
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level > 0:
                private = [a.name for a in node.names if a.name.startswith('_') and
                           not (node.module is None and a.name in ('_lib', '_device'))]
                assert not private, (mod, node.lineno, private)


@pytest.mark.parametrize('home, names', [('selection', SELECTION), ('_device', DEVICE)])
def test_every_moved_name_has_one_home(home, names):
    for name in names:
        where = [mod for mod, tree in TREES.items() if name in _defined(tree)]
        assert where == [home], (name, where)


def test_selection_is_plain_numpy():
    """No import, at any depth, of torch, ctypes or anything of the package."""
    for node in ast.walk(TREES['selection']):
        if isinstance(node, ast.ImportFrom):
            assert node.level == 0, node.lineno
            roots = [(node.module or '').split('.')[0]]
        elif isinstance(node, ast.Import):
            roots = [a.name.split('.')[0] for a in node.names]
        else:
            continue
        assert not set(roots) & {'torch', 'ctypes', 'bayhunter_amd'}, (node.lineno, roots)


def test_the_upload_preamble_is_written_once():
    """posterior and moho raise nothing of their own about the shape of `models` or the number of weights."""
    for mod in ('posterior', 'moho'):
        src = open(os.path.join(PKG, mod + '.py')).read()
        for words in ('2*maxlayers]")', 'per row")'):
            assert words not in src, (mod, words)
    src = open(os.path.join(PKG, '_device.py')).read()
    assert src.count('2*maxlayers]")') == 1 and 'ValueError(per_row)' in src


def test_statistic_modules_expose_no_moved_name():
    """The three refer to the two lower layers by module (sel.*, _device.*): no moved name is an attribute of theirs,
    under its new name or its old one."""
    old = ('_NO_BEST_CHAIN', '_Handle', '_torch_device', '_to_device', '_rows_weights', '_Fits', '_Grid', '_Sets')
    for mod in STATISTICS:
        m = importlib.import_module('bayhunter_amd.' + mod)
        for name in SELECTION + DEVICE + old:
            assert not hasattr(m, name), (mod, name)
    chains = open(os.path.join(PKG, 'chains.py')).read()
    assert 'from .selection import pool_outliers' in chains and 'from .posterior import pool_outliers' not in chains
