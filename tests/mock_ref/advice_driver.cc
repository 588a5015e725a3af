// tests/mock_ref/advice_driver.cc -- the advice move through include/gaml_hip_prob_calculator.h, compiled against the
// declaration mock in this directory. ExtendPathsAdv below is moves.cc:933-998 with the patch of INTEGRATION.md §7
// applied: the lines between the BEGIN / END markers are the patch's new text (tests/test_gpu_advice_adapter.py
// compares the two), so the documented patch is the code this driver runs.
//   advice_driver <LastGraph> <fastq1> <fastq2> <insert_mean> <insert_std> <threshold> <seed> <moves> [<single fastq>]
// Scores the genome walk once (GAML scores before it moves), then makes <moves> advice moves on stretches of the walk
// and prints one line per move: the path, only_out, allow_gaps after the retry, the candidate list.
// reach_limit_[v] (gaml.cc:99, 299-300 fills it from the reads) holds here the nodes v + 2, v + 4, ..., v + 16 modulo
// the node count.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "gaml_hip_prob_calculator.h"

string gBlasrPath = "blasr/alignment/bin";  // gaml.cc:30

struct AdviceGraph : Graph {  // the member of the reference's Graph the advice move reads (graph.h:244)
  vector<unordered_map<int, vector<int> > > reach_limit_;
};

// moves.cc:933-998 up to the choice of the next node; returns the candidate list (the reference draws from it next)
static vector<int> ExtendPathsAdv(vector<int> path, AdviceGraph& gr, int threshold, ReadSet& rs1, ReadSet& rs2, ProbCalculator& prob_calc,
                                  vector<int>* path_out, bool* only_out_out, bool* allow_gaps_out) {
  int rev = rand() % 2;  // moves.cc:938-945
  if (rev == 1) {
    for (int i = 0; i < (int)path.size(); i++)
      if (path[i] >= 0) path[i] ^= 1;
    reverse(path.begin(), path.end());
  }
  // BEGIN moves.cc:948-986 as patched
  vector<int> cands;
  bool only_out = true;
  if (rand() % 5 == 0) only_out = false;
  bool allow_gaps = false;
  if (rand() % 5 == 0) allow_gaps = true;
  vector<int> reach;
  for (auto& e : gr.reach_limit_[path.back()]) reach.push_back(e.first);
  prob_calc.AdviceCandidates(rs1, rs2, threshold, path, only_out, allow_gaps, reach, cands);
  if (cands.empty()) {
    allow_gaps = true;
    prob_calc.AdviceCandidates(rs1, rs2, threshold, path, only_out, allow_gaps, reach, cands);
  }
  // END
  *path_out = path;
  *only_out_out = only_out;
  *allow_gaps_out = allow_gaps;
  return cands;
}

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: advice_driver LastGraph fq1 fq2 mean std threshold seed moves [single.fq]\n"); return 2; }
  AdviceGraph gr;
  if (!gr.Load(argv[1])) { fprintf(stderr, "cannot load %s\n", argv[1]); return 1; }
  const double mean = atof(argv[4]), sd = atof(argv[5]);
  const int threshold = atoi(argv[6]), moves = atoi(argv[8]);
  srand((unsigned)atoi(argv[7]));
  const int n = (int)gr.nodes.size();
  gr.reach_limit_.resize(n);
  for (int v = 0; v < n; v++)
    for (int k = 1; k <= 8; k++) gr.reach_limit_[v][(v + 2 * k) % n].push_back(0);
  vector<pair<SingleReadConfig, ReadSet*> > single_reads;
  vector<pair<PairedReadConfig, pair<ReadSet*, ReadSet*> > > paired_reads;
  vector<pair<SingleReadConfig, PacbioReadSet*> > pacbio_reads;
  ReadSet* r1 = new ReadSet("a1", argv[2], 0.96, 0.01);
  ReadSet* r2 = new ReadSet("a2", argv[3], 0.96, 0.01);
  paired_reads.push_back(make_pair(PairedReadConfig(0, mean - 50, mean, sd, -0.7, -10, 1, true), make_pair(r1, r2)));
  if (argc > 9) single_reads.push_back(make_pair(SingleReadConfig(0, 50, -0.7, -10, 0.5, false), new ReadSet("s", argv[9], 0.96, 0.01)));
  ProbCalculator pc(single_reads, paired_reads, pacbio_reads, gr);
  vector<vector<int> > whole(1);
  for (int i = 0; i < n; i += 2) whole[0].push_back(i);
  printf("whole %.17g\n", pc.CalcProb(whole));
  const int w = (int)whole[0].size();
  for (int k = 0; k < moves; k++) {
    const int a = (7 * k) % w, len = 2 + k % 9;
    vector<int> path(whole[0].begin() + a, whole[0].begin() + std::min(w, a + len)), used;
    bool only_out = false, allow_gaps = false;
    vector<int> cands = ExtendPathsAdv(path, gr, threshold, *r1, *r2, pc, &used, &only_out, &allow_gaps);
    printf("move %d path", k);
    for (size_t i = 0; i < used.size(); i++) printf(" %d", used[i]);
    printf(" flags %d %d cands %d", (int)only_out, (int)allow_gaps, (int)cands.size());
    for (size_t i = 0; i < cands.size(); i++) printf(" %d", cands[i]);
    printf("\n");
  }
  return 0;
}
