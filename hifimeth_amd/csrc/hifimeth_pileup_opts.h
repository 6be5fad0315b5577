// hifimeth_pileup_opts.h -- the command lines of `hifimeth-hip pileup`, `diff`, `groupdiff`, `samplecorr`, `regiondiff`, `groupdmr` and `smooth`: the options as the rest of the
// front end reads them, and one call that parses, checks and reports (hifimeth_pileup_opts.cpp holds the option table, which is
// also the usage text, and the ordered list of checks).  Host code without the engine: nothing here opens a file or a device.
#pragma once

#include <cstdint>
#include <string>

// One field per flag, grouped by output; the option table says what each flag means.  An output is on when its first field is set.
struct PileupOptions {
    int min_mapq = 0, threads = 8, device = 0, read_batch = 512;  // -q -t -d -b
    double min_pi = 0.0;                                           // -f
    bool haplotypes = false, asm_test = false, asm_q = false, asm_regions = false;  // -H -A -Q -G
    int asm_min_cov = 5, region_min_loci = 3;                      // -a -n
    double region_max_p = 0.01;                                    // -s
    long long region_max_gap = 500;                                // -g
    std::string control;                                           // -B: the control sequence whose rates are measured
    bool rates_given = false;                                      // -e: the three rates given directly (NaN: context not tested)
    double rates[3] = {0, 0, 0};
    bool domains = false;                                          // -D
    double domain_lo[3] = {0.1, 0.05, 0.02}, domain_hi[3] = {0.8, 0.5, 0.2}, domain_penalty = 8.0;  // -u (NaN: not segmented) -x
    int64_t dom_A[3] = {0, 0, 0}, dom_B[3] = {0, 0, 0}, dom_S = 0;  // the integer weights of the levels (hm_domain_scores)
    long long domain_max_gap = 1000, domain_fit_iter = 0;          // -j -Y (0: no fit)
    int patterns = 0;                                              // -E (0: off)
    long long pattern_span = 150, pattern_min_reads = 10;          // -w -o
    bool bedmethyl = false;                                        // -M
    long long bedmethyl_min_valid = 1;                             // -v
    long long linkage = 0, linkage_min_pairs = 1;                  // -L (0: off) -z
    long long profile = 0, profile_min_calls = 1, trim5 = 0, trim3 = 0;  // -P (0: off) -y -I
    std::string intervals;                                         // -R
    long long interval_min_cov = 1, meta_flank = 0;                // -C, -J bins[:flank:flank_bins]
    int meta_bins = 0, meta_flank_bins = 0;
    int context_flank = -1;                                        // -S (-1: off)
    long long context_min_cov = 1;                                 // -O
    bool kinetics = false;                                         // -K: call on the fly, with `call`'s options
    std::string model_dir;                                         // -m, default <exe_dir>/../weights
    int ctx_mask = 7, min_read_size = 1000, precision = 1, trunk = -1;  // -c -l -p -T (-1: the call engine decides per context)
    long long group_min_cov = 5, group_min_reps = 2;               // groupdiff -a -r, groupdmr -a -r
    double dmr_max_p = 0.01, dmr_max_q = 0.0, dmr_min_diff = 0.0;  // groupdmr -s -F (0: chain by p) -m
    long long dmr_max_gap = 500, dmr_min_loci = 3;                 // groupdmr -g -n
    bool dmr_loci = false;                                         // groupdmr -L
    long long sample_min_cov = 5;                                  // samplecorr -a -k
    bool sample_complete = false;
    long long region_min_sample_loci = 3, region_min_reps = 2;     // regiondiff -l -r (its -R -a -k: intervals, sample_min_cov, sample_complete)
    long long smooth_half_width = 500, smooth_min_cov = 1, smooth_min_loci = 1;  // smooth -W -a -i
    std::string ref, bam, prefix;
};

enum Command { CMD_PILEUP = 1, CMD_DIFF = 2, CMD_GROUPDIFF = 4, CMD_SAMPLECORR = 8, CMD_REGIONDIFF = 16, CMD_GROUPDMR = 32, CMD_SMOOTH = 64 };

// The whole text as a decimal integer in [lo, hi] -> out, true.  Leading blanks and a sign pass, as strtoll takes them; an empty
// text, anything behind the number and a value beyond long long do not, and leave `out` alone.
bool whole_int(const char* text, long long lo, long long hi, long long& out);
// The whole text as a double -> out, true; the same rules, a result out of double's range (ERANGE) fails.  The caller checks the range.
bool whole_double(const char* text, double& out);

// Parses the options of `cmd` from argv[2] on and runs the checks.  true: go on, the positional arguments start at argv[first]
// (3 for pileup, samplecorr and smooth, 4 for diff, groupdiff, regiondiff and groupdmr).  false: the usage, behind an error message if there is one, has been printed; leave with `status`
// (0 after -h).  levels_ok turns the levels and penalty of -D into o's integer weights, false if they give none: the one check
// that needs the library, so pileup brings it.  It runs once the options have parsed, ahead of the rules; it only writes the weights.
// the usage of `cmd` on stderr, as parse_command_line prints it: for what a command finds wrong with its positional arguments
void command_usage(Command cmd, const char* exe);
bool parse_command_line(Command cmd, int argc, char** argv, PileupOptions& o, int& first, int& status, bool (*levels_ok)(PileupOptions&) = nullptr);
