"""host/LocalMapping_shim.h with SearchInNeighborsChain (both Fuse directions of LocalMapping::SearchInNeighbors on dvm_fuse_targets)
must compile against the reference's signatures: the recipe of tests/test_shims_compile.py -- `g++ -fsyntax-only -Wall -Werror` with the
mock classes under tests/stubs/ -- on a translation unit that INSTANTIATES the function, with the default seam and with a test's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dvm_slam_amd", "host")

USE = r'''
#include "LocalMapping_shim.h"
int use(ORB_SLAM3::KeyFrame* keyFrame, std::vector<ORB_SLAM3::KeyFrame*>& vpTargetKFs, bool& mbAbortBA) {
  const ORB_SLAM3::SearchInNeighborsCounts fused = ORB_SLAM3::SearchInNeighborsChain(keyFrame, vpTargetKFs, &mbAbortBA);
  if (fused.aborted) return -1;
  int replaces = 0;
  const ORB_SLAM3::SearchInNeighborsCounts again =
      ORB_SLAM3::SearchInNeighborsChain(keyFrame, vpTargetKFs, nullptr, [&](ORB_SLAM3::MapPoint* survivor, ORB_SLAM3::MapPoint* replaced) {
        replaces += survivor != replaced;
      });
  int n = fused.nFusedCurrent + fused.nDeviceCalls + again.nDeviceCalls + replaces;
  for (int f : fused.nFused) n += f;
  return n;
}
int main() { return 0; }
'''


def test_search_in_neighbors_chain_compiles_against_reference_signatures():
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tests", "stubs"),
                        "-I", os.path.join(ROOT, "include"), "-I", HOST, "-x", "c++", "-"], input=USE, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_header_shows_the_rewritten_function():
    txt = open(os.path.join(HOST, "LocalMapping_shim.h")).read()
    for needle in ("SearchInNeighborsChain(keyFrame, vpTargetKFs, &mbAbortBA)", "mnFuseCandidateForKF", "UpdateConnections", "NLeft != -1"):
        assert needle in txt, needle
