"""Host side of the batched preprocessing (csrc/bfs_blocks.hip): the entry points are exported, declared and bound under ABI 51; the
structs match the header; what the kernels do not cover is refused before any HIP call; the workspace query is the Python formula;
the Python entry points' argument checks; the bound covers every graph the one-launch routes and config C2 hold.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from gnan_amd import HopGraph, _lib, graph
from gnan_amd import small_graph as sg
from conftest import ROOT

SYMBOLS = ("gnan_bfs_blocks", "gnan_shell_counts_blocks", "gnan_bfs_blocks_workspace_bytes")
STRUCTS = (("gnan_bfs_blocks_args", "BfsBlocksArgs"), ("gnan_shell_counts_blocks_args", "ShellCountsBlocksArgs"))
BOUND = _lib.BFS_BLOCKS_MAX_NODES


def header():
    with open(os.path.join(ROOT, "include", "gnan_hip.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound_under_abi_51():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    number = int(re.search(r"^#define GNAN_ABI_VERSION (\d+)$", header(), re.M).group(1))
    assert _lib.lib().gnan_abi_version() == _lib.ABI_VERSION == number == 51
    assert int(re.search(r"^#define GNAN_BFS_BLOCKS_MAX_NODES (\d+)$", header(), re.M).group(1)) == BOUND


def test_struct_layouts_match_the_header():
    """The parser check of test_abi.py::test_struct_layout_matches_header, with the types, for the new structs."""
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t}
    for struct, cls_name in STRUCTS:
        cls = getattr(_lib, cls_name)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            words = decl.replace("const ", "").split(None, 1)
            for name in words[1].split(","):
                name = name.strip()
                pointer = name.startswith("*") or words[0].endswith("*")
                fields.append((name.lstrip("*").strip(), ctypes.c_void_p if pointer else c_types[words[0]]))
        assert fields == list(cls._fields_), struct


def _sizes(values):
    return (ctypes.c_int32 * len(values))(*values)


def _args(graph_sizes=(5, 70), **over):
    """gnan_bfs_blocks_args of made-up (never dereferenced) device addresses and a real host size list."""
    host = _sizes(graph_sizes)
    need = _lib.lib().gnan_bfs_blocks_workspace_bytes(host, len(graph_sizes))
    kw = dict(src=0x100000, dst=0x200000, n_edges=10, graph_of=0x300000, n_nodes=sum(graph_sizes), node_off=0x400000, code_off=0x500000,
              bit_off=0x600000, tile_graph=0x700000, tile_src=0x800000, sizes=ctypes.addressof(host), n_tiles=3, n_graphs=len(graph_sizes),
              max_nodes=max(graph_sizes), max_hops=255, code=0x900000, max_hop=0xA00000, status=0xB00000, workspace=0xC00000,
              workspace_bytes=need)
    kw.update(over)
    a = _lib.BfsBlocksArgs(**kw)
    a._keep = host
    return a


def _count_args(**over):
    kw = dict(code=0x100000, graph_of=0x200000, n_nodes=75, node_off=0x300000, code_off=0x400000, cnt_off=0x500000, max_hop=0x600000,
              n_graphs=2, max_nodes=70, cnt=0x700000)
    kw.update(over)
    return _lib.ShellCountsBlocksArgs(**kw)


def test_refusals_come_before_any_hip_call():
    """A null stream and made-up addresses on a machine without a device: every answer is the host-side checks'."""
    lib = _lib.lib()
    assert lib.gnan_bfs_blocks(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    assert lib.gnan_shell_counts_blocks(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
    for field in ("graph_of", "node_off", "code_off", "bit_off", "sizes", "max_hop", "status", "workspace", "src", "dst", "tile_graph",
                  "tile_src", "code"):
        assert lib.gnan_bfs_blocks(_args(**{field: None}), None) == _lib.ERR_BAD_ARG, field
        assert b"null" in lib.gnan_last_error(), field
    for field in ("code", "graph_of", "node_off", "code_off", "cnt_off", "max_hop", "cnt"):
        assert lib.gnan_shell_counts_blocks(_count_args(**{field: None}), None) == _lib.ERR_BAD_ARG, field
        assert b"null pointer" in lib.gnan_last_error(), field
    assert lib.gnan_bfs_blocks(_args(max_hops=0), None) == _lib.ERR_BAD_ARG and b"max_hops" in lib.gnan_last_error()
    assert lib.gnan_bfs_blocks(_args(n_edges=-1), None) == _lib.ERR_BAD_ARG
    # beyond the cover: the limit and the value, by name
    for call, a in ((lib.gnan_bfs_blocks, _args(max_nodes=BOUND + 1)), (lib.gnan_shell_counts_blocks, _count_args(max_nodes=BOUND + 1))):
        assert call(a, None) == _lib.ERR_UNSUPPORTED
        msg = lib.gnan_last_error()
        assert b"at most %d nodes" % BOUND in msg and b"max_nodes=%d" % (BOUND + 1) in msg, msg
    # a workspace one byte short: both sizes
    need = lib.gnan_bfs_blocks_workspace_bytes(_sizes((5, 70)), 2)
    assert need == 8 * (5 * 1 + 70 * 2)
    assert lib.gnan_bfs_blocks(_args(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
    assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
    # nothing to do
    assert lib.gnan_bfs_blocks(_args(n_graphs=0), None) == 0
    assert lib.gnan_shell_counts_blocks(_count_args(n_graphs=0), None) == 0
    assert lib.gnan_shell_counts_blocks(_count_args(n_nodes=0), None) == 0


@pytest.mark.parametrize("sizes", [[1], [64, 65], [448], [0, 5, 0], [BOUND, BOUND + 1]])
def test_workspace_query_is_the_python_formula(sizes):
    want = 8 * sum(n * -(-n // 64) for n in sizes if n <= BOUND)
    assert graph.bfs_blocks_workspace_bytes(sizes) == want
    assert _lib.lib().gnan_bfs_blocks_workspace_bytes(_sizes(sizes), len(sizes)) == want


def test_packed_offsets():
    assert graph.packed_offsets([]) == [0]
    assert graph.packed_offsets([3, 0, 5]) == [0, 3, 3, 8]
    assert graph.packed_offsets([1, 16, 17, 0, 4], 16) == [0, 16, 32, 64, 64, 80]
    assert graph.BFS_BLOCKS_ALIGN % 4 == 0        # gnan_mid_graph_fwd wants 4-byte aligned code rows


def test_python_argument_checks():
    ei, batch = torch.tensor([[0, 1], [1, 0]]), torch.tensor([0, 0])
    with pytest.raises(_lib.GnanHipError, match="no CPU fallback"):
        HopGraph.batch_from_edge_index(ei, batch)
    for bad in (1, 0, -3, 2.5):
        with pytest.raises(ValueError, match="max_hops"):
            HopGraph.batch_from_edge_index(ei, batch, max_hops=bad)
    from gnan_amd.batched import HopBlocks, collate_edges
    with pytest.raises(_lib.GnanHipError, match="no CPU fallback"):
        HopBlocks.from_edge_index(ei, batch)
    with pytest.raises(_lib.GnanHipError, match="no CPU fallback"):
        collate_edges([(torch.rand(2, 3), ei, torch.tensor([1]))])
    import gnan_amd

    class Bag:
        pass

    d = Bag()
    d.x, d.edge_index = torch.rand(2, 3), ei
    with pytest.raises(_lib.GnanHipError, match="no CPU fallback"):
        gnan_amd.attach_hop_graphs([d])
    assert gnan_amd.attach_hop_graphs([]) == []
    assert "attach_hop_graphs" in gnan_amd.__all__


def test_the_bound_covers_the_one_launch_routes_and_config_c2():
    assert BOUND >= sg.MID_GRAPH_MAX_NODES >= sg.SMALL_GRAPH_MAX_NODES
    assert BOUND >= 448
    from gnan_amd import synthetic
    sizes = [int(x.shape[0]) for _, x, _ in synthetic.mutagenicity_shaped_graphs(4337, seed=0)]
    assert len(sizes) == 4337 and max(sizes) <= BOUND          # no C2 graph takes the per-graph route
    # LDS of the BFS workgroup at the bound: n rows of an ODD number of 64-bit words — four workgroups to a compute unit
    assert BOUND * (-(-BOUND // 64) | 1) * 8 <= 40 * 1024
