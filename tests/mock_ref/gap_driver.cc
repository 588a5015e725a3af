// tests/mock_ref/gap_driver.cc -- the gap-length search through include/gaml_hip_prob_calculator.h, compiled against the
// declaration mock in this directory. FixGapLength below is moves.cc:729-800 with the patch of INTEGRATION.md §8
// applied: the lines between the BEGIN / END markers are the patch's text (tests/test_gap_host.py compares the two), so
// the documented patch is the code this driver runs.
//   gap_driver <LastGraph> <fastq1> <fastq2> <insert_mean> <insert_std> <site> <start> [<site> <start> ...]
// Scores the genome walk once (GAML scores before it moves). Then, per (site, start): the walk with the node at
// position <site> replaced by a gap of <start> bases, beside the short path walk[3..9), goes through the search; one
// line per search: site, start, the length the search leaves in the entry.
#include <cstdio>
#include <cstdlib>

#include "gaml_hip_prob_calculator.h"

string gBlasrPath = "blasr/alignment/bin";  // gaml.cc:30

// BEGIN moves.cc:729-800 as patched
bool FixGapLength(vector<vector<int> >& paths, int path_id, int gap_pos,
                  ProbCalculator& prob_calc, int prev_len) {
  return prob_calc.FixGapLength(paths, path_id, gap_pos);
}
// END

int main(int argc, char** argv) {
  if (argc < 8 || (argc - 6) % 2 != 0) { fprintf(stderr, "usage: gap_driver LastGraph fq1 fq2 mean std site start [site start ...]\n"); return 2; }
  Graph gr;
  if (!gr.Load(argv[1])) { fprintf(stderr, "cannot load %s\n", argv[1]); return 1; }
  const double mean = atof(argv[4]), sd = atof(argv[5]);
  vector<pair<SingleReadConfig, ReadSet*> > single_reads;
  vector<pair<PairedReadConfig, pair<ReadSet*, ReadSet*> > > paired_reads;
  vector<pair<SingleReadConfig, PacbioReadSet*> > pacbio_reads;
  ReadSet* r1 = new ReadSet("a1", argv[2], 0.96, 0.01);
  ReadSet* r2 = new ReadSet("a2", argv[3], 0.96, 0.01);
  paired_reads.push_back(make_pair(PairedReadConfig(0, 50, mean, sd, -0.7, -10, 1, true), make_pair(r1, r2)));
  ProbCalculator pc(single_reads, paired_reads, pacbio_reads, gr);
  vector<vector<int> > whole(1);
  for (int i = 0; i < (int)gr.nodes.size(); i += 2) whole[0].push_back(i);
  printf("whole %.17g\n", pc.CalcProb(whole));
  for (int a = 6; a + 1 < argc; a += 2) {
    const int site = atoi(argv[a]), start = atoi(argv[a + 1]);
    if (site < 0 || site >= (int)whole[0].size() || start < 1 || whole[0].size() < 9) { fprintf(stderr, "bad site / start\n"); return 2; }
    vector<vector<int> > paths(2);
    paths[0] = whole[0];
    paths[0][site] = -start;
    paths[1].assign(whole[0].begin() + 3, whole[0].begin() + 9);
    FixGapLength(paths, 0, site, pc, -1);
    printf("gap %d %d -> %d\n", site, start, -paths[0][site]);
  }
  return 0;
}
