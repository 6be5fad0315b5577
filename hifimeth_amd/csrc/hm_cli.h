// hm_cli.h -- the commands of hifimeth-hip outside hifimeth_call.cpp, which dispatches to them, and what two of their files share
#pragma once

#include <cstdint>
#include <vector>

#include "hm_bam.h"

int cmd_pileup(int argc, char** argv);  // hifimeth_pileup.cpp
int cmd_diff(int argc, char** argv);
int cmd_groupdiff(int argc, char** argv);
int cmd_samplecorr(int argc, char** argv);
int cmd_regiondiff(int argc, char** argv);
int cmd_groupdmr(int argc, char** argv);
int cmd_smooth(int argc, char** argv);
int cmd_corr(int argc, char** argv);  // hifimeth_tools.cpp
int cmd_cov2bed(int argc, char** argv);
int cmd_sample(int argc, char** argv);
int cmd_eval(int argc, char** argv);
int cmd_fastats(int argc, char** argv);
int cmd_thresholds(int argc, char** argv);

// hifimeth_pileup.cpp; `eval` reads alignments and thresholds as `pileup` does
void real_cigar(const hmbam::BamRecord& r, std::vector<uint32_t>& cig);
void report_thresholds(const uint64_t* bins, uint8_t thr[3]);
