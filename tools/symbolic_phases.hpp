// The phases of build_symbolic (csrc/symbolic_build.hpp) and of the nested dissection (csrc/ordering_build.hpp), compiled INTO a developer tool: libfgo builds them as translation units of their
// own (build.py FGO_SOURCES), a tool takes them through this header, so that its build line stays the one it always had --
//   g++ -O2 -std=c++17 -pthread -I.. <tool>.cpp ../graph_slam_amd/csrc/symbolic.cpp ../graph_slam_amd/csrc/ordering.cpp ../graph_slam_amd/csrc/synth.cpp
// -- and does not have to follow the file lists of the two phases.  Include it from ONE source of the tool and do not put the
// phase files on the command line as well.
#pragma once
#include "../graph_slam_amd/csrc/symbolic_pattern.cpp"
#include "../graph_slam_amd/csrc/symbolic_schedule.cpp"
#include "../graph_slam_amd/csrc/symbolic_lists.cpp"
#include "../graph_slam_amd/csrc/symbolic_panels.cpp"
#include "../graph_slam_amd/csrc/symbolic_riders.cpp"
#include "../graph_slam_amd/csrc/ordering_cuts.cpp"
#include "../graph_slam_amd/csrc/ordering_leaves.cpp"
#include "../graph_slam_amd/csrc/ordering_tree.cpp"
