// sample_set_check -- the sample-set front and the owning output file of hifimeth_pileup.cpp (host only), as a stand-alone program
// that host sanitizers can watch: one list and two, an empty element, too few and too many samples, the echo, a path that cannot be
// written, files closed by scope and by assignment.  The unit under test is included, the rest of the CLI linked, e.g.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/sample_set_check.cpp hifimeth_amd/csrc/hifimeth_pileup_opts.cpp \
//       hifimeth_amd/csrc/hifimeth_tools.cpp hifimeth_amd/csrc/hm_bam.cpp -Lhifimeth_amd -lhifimeth_hip -lz -ldl -pthread \
//       -Wl,-rpath,$PWD/hifimeth_amd -o sample_set_check && ./sample_set_check /tmp
// No device is touched: it runs on a machine without a GPU.  The messages of the refused sets go to stderr.
#include "../hifimeth_amd/csrc/hifimeth_pileup.cpp"

static int bad = 0;
#define CHECK(x) \
    do { \
        if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++bad; } \
    } while (0)

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "USAGE: %s writable-directory\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    {  // one list
        const SampleSet set("a,b,c");
        CHECK(set.lists == 1 && set.sample == (std::vector<std::string>{"a", "b", "c"}) && set.group[1].empty());
        CHECK(set.member == std::vector<uint8_t>(3, 1));
        CHECK(set.count_fits(CMD_SAMPLECORR, "samplecorr", 2, argv[0]) && set.lists_fit(0, 0));
        set.echo();
    }
    {  // two lists
        const SampleSet set("a,b", "c,d,e");
        CHECK(set.lists == 2 && set.sample.size() == 5 && set.group[0].size() == 2 && set.group[1].size() == 3 && set.sample[2] == "c");
        CHECK(set.member == (std::vector<uint8_t>{1, 1, 2, 2, 2}));
        CHECK(set.count_fits(CMD_REGIONDIFF, "regiondiff", 0, argv[0]) && set.lists_fit(2, 255));
        CHECK(!set.lists_fit(3, 0));    // group 1 has fewer than -r 3
        CHECK(!set.lists_fit(2, 2));    // group 2 has more than 2
        set.echo();
    }
    // an empty element: in the middle, at either end, the whole list
    CHECK(!SampleSet("a,,b").lists_fit(0, 0) && !SampleSet(",a").lists_fit(0, 0) && !SampleSet("a,").lists_fit(0, 0) && !SampleSet("").lists_fit(0, 0));
    CHECK(!SampleSet("a,b", "c,,d").lists_fit(2, 0) && SampleSet("").sample.size() == 1);
    // too few and too many
    CHECK(!SampleSet("a").count_fits(CMD_SAMPLECORR, "samplecorr", 2, argv[0]));
    std::string many = "s0";
    for (int i = 1; i < HM_SAMPLE_MAX; ++i) many += ",s" + std::to_string(i);
    CHECK(SampleSet(many.c_str()).count_fits(CMD_SAMPLECORR, "samplecorr", 2, argv[0]));
    CHECK(!SampleSet((many + ",x").c_str()).count_fits(CMD_SAMPLECORR, "samplecorr", 2, argv[0]));
    CHECK(!SampleSet(many.c_str(), "x").count_fits(CMD_REGIONDIFF, "regiondiff", 0, argv[0]));
    // the owning file: a path that cannot be written, files closed by scope, by assignment and by release
    CHECK(!open_out(dir + "/no-such-directory/x.tsv"));
    {
        CtxFiles none;
        CHECK(!none.open(dir + "/no-such-directory/p", "t.", ".bed"));
    }
    const std::string prefix = dir + "/sample_set_check";
    {
        CtxFiles out;
        CHECK(out.open(prefix, "t.", ".bed"));
        for (int c = 0; c < 3; ++c) CHECK(out.f[c] && fprintf(out.f[c], "%s\n", CTX_NAME[c]) > 0);
        OutFile f = open_out(prefix + ".one.tsv");
        CHECK(f && fputs("1\n", f.get()) >= 0);
        f = open_out(prefix + ".two.tsv");
        CHECK(f && fputs("2\n", f.get()) >= 0 && fclose(f.release()) == 0 && !f);
    }
    for (const char* tail : {".t.CpG.bed", ".t.CHG.bed", ".t.CHH.bed", ".one.tsv", ".two.tsv"}) {
        FILE* f = fopen((prefix + tail).c_str(), "rb");
        char line[8] = "";
        CHECK(f && fgets(line, sizeof line, f) && strlen(line) >= 2);  // written and flushed by the close
        if (f) fclose(f);
        remove((prefix + tail).c_str());
    }
    printf("sample_set_check: %d failed\n", bad);
    return bad ? 1 : 0;
}
