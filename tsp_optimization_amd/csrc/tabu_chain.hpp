// tabu_chain.hpp -- the words of tsp_dev_tours::d_chain: what a chain of tabu() iterations (tsp_grid_tabu_iterations) shares
// between the host, k_tabu_post_chain (queued chains) and k_cluster_two_opt (iterations inside the launch).  All ints.
#pragma once

namespace tsp {

constexpr int kMaxChain = 128;   // iterations of one chain
constexpr int kMaxPairs = 256;   // host-drawn kick trials of one chain

constexpr int kChainStop = 0;     // set on the device: every later launch (iteration) of the chain is a no-op
constexpr int kChainResume = 1;   // in-kernel chains: the iteration the next launch goes on with
constexpr int kChainBest = 2;     // the incumbent's cost (double: words 2 .. 3)
constexpr int kChainRes = 4, kChainResWords = 10;   // then the result words of every iteration, indexed by kRes*:
constexpr int kResAccepted = 0, kResA1 = 1, kResB1 = 2;   // the kick's last trial, as k_tabu_kick reports it
constexpr int kResTrials = 3;     // in-kernel chains: kick trials taken
constexpr int kResRan = 4, kResImproved = 5;   // the iteration ran to its kick's trial; its tour became the incumbent
constexpr int kResWhy = 6;        // 1: the descent did not finish in its launch, or the exchange gave up
constexpr int kResCost = 8;       // the finished tour's cost (double: words 8 .. 9)
// in-kernel chains, behind the results: the tenure per iteration, {a, b, a and b in rank order} per kick trial, the index of
// the next trial
constexpr int kChainPar = kChainRes + kChainResWords * kMaxChain, kChainAb = kChainPar + kMaxChain, kChainPp = kChainAb + 4 * kMaxPairs;
constexpr int kChainInts = kChainPp + 4;

}  // namespace tsp
