"""bundleadjustment_amd — MI355X-native replacement for the Ceres Problem/Solve
bundle-adjustment path of MatteoWohlrapp/BundleAdjustment.

The numeric work runs in hand-written HIP kernels for gfx950 behind the C-ABI
of include/ba_hip.h (libba_hip.so).  This package is the thin host side:
ctypes binding, problem container, synthetic problem generator, and the
optimizer classes that mirror the reference's API (Optimizer.h:196-289).
"""
from .problem import (AssocBatch, IcpBatch, pack_icp_batch, MapGraphResult, MapPointBatch, MapTable, MatchBatch, map_table_from_problem, windows_from_graph, Problem, TriangulationBatch, WindowBatch, make_config, make_synthetic,  # noqa: F401
                      pack_assoc_batch, pack_map_point_batch, pack_match_batch, pack_window_batch, shard_points,
                      triangulation_batch, HUBER_A)
from ._native import BAError  # noqa: F401
from .solver import Options, Solver, Summary, solve  # noqa: F401

__all__ = ["AssocBatch", "IcpBatch", "pack_icp_batch", "MapGraphResult", "MapPointBatch", "MapTable", "map_table_from_problem", "windows_from_graph", "MatchBatch", "pack_assoc_batch", "pack_map_point_batch", "Problem", "TriangulationBatch", "WindowBatch", "make_config", "make_synthetic", "pack_match_batch",
           "pack_window_batch",
           "shard_points", "triangulation_batch", "HUBER_A", "Options", "Solver", "Summary", "solve", "BAError"]
