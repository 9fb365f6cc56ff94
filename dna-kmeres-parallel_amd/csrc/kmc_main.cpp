// kmc_main.cpp — the C++ host driver: successor of the reference program's main()
// (main.cu:120-174) and its GPU driver doParallelKmereDistance (main.cu:215-399),
// calling the HIP kernels only through the C ABI of include/kmc.h.
//
// Flow (the reference's, with its hard-coded constants turned into options):
//   importSeqs / importSeqsNoNL           -> kmc_fasta_load_device (file -> HBM, parsed on the GPU;
//                                            --host-loader: kmc_fasta_load) (main.cu:163, 474-545 / 401-473)
//   step 1: sumKmereCoincidencesGlobalMemory -> kmc_count_dense / kmc_count_multi
//                                               (--dropin: sumKmereCoincidencesGlobalMemory_hip)
//                                                                    (main.cu:287-300)
//   step 2: n x minKmeres2 launches       -> kmc_pair_distances, one launch
//                                               (--dropin: n x minKmeres2_hip) (main.cu:326-344)
//   parallel_results.csv, "%f\n" per entry of the packed upper triangle (main.cu:351-358),
//   and sequential_results.csv, the CPU path's distances (main.cu:194-202)
// and the step-1 / step-2 / total event timers the reference prints.  Extras:
// a histogram dump (--counts, F3 of SURVEY.md §8(f)), k up to 13 (the reference
// kernel is k = 3 only), multi-GPU counting over RCCL (--gpus), canonical k <= 31
// counting (--canonical), and with it step 2 on the sparse counts (--distances:
// kmc_pair_distances_sparse) or on MinHash sketches of them (--sketch:
// kmc_sketch_from_counts + kmc_sketch_distances -> sketch_results.csv; --sketch-direct:
// kmc_sketch_from_sequences instead, no canonical count; --per-file: one sketch per input file,
// kmc_sketch_from_sequences_grouped; --query FILE: the input files are references that FILE's
// sketches are searched in, kmc_sketch_nearest -> query_results.tsv, or with --top 0
// kmc_sketch_distances_rect -> query_distances.csv; --screen FILE: the input files are references
// looked for among all k-mers of FILE, a read set or metagenome, kmc_sketch_screen_* ->
// screen_results.tsv; --winner-takes-all: kmc_sketch_screen_winners' lines instead of _results').  Inputs may be FASTQ (--format, or a .fq / .fastq name):
// kmc_fastq_load_device, and a --screen FILE in FASTQ is streamed batch by batch
// (kmc_fastq_open / _next / _close), so its size is not bounded by device memory.
// --per-file --min-abundance M: every file is one pass of the abundance accumulator
// (kmc_sketch_accum_*), a FASTQ file streamed the same way; --spectrum B: that pass's abundance
// spectrum (kmc_spectrum_from_accum, kmc_spectrum_summarize -> spectrum.tsv, spectrum_summary.tsv),
// from which --min-abundance auto takes every file's M.  --cluster D: the sketches, however
// made, are grouped at Mash distance D (kmc_sketch_cluster -> clusters.tsv) instead of compared.
// --pairs D: the pairs of sketches within Mash distance D with their counts and distances
// (kmc_sketch_links -> pairs.tsv; with --query FILE kmc_sketch_links_rect -> query_pairs.tsv)
// instead of every distance.  --recruit FILE: the input files are one k-mer set in the accumulator
// and every record of FILE is matched against it (kmc_match_from_accum -> read_matches.tsv,
// read_matches_summary.tsv); --write-recruited / --write-rest: the listed records, or the others, as
// the raw FASTQ text of the input (kmc_match_select, kmc_select_records on the reader's raw batch ->
// recruited_<f>.fastq, rest_<f>.fastq).  --classify: every input file is one source; after the adds
// the inputs are read again and labelled (kmc_label_accum), and the match becomes
// kmc_classify_from_accum -> read_sources.tsv, read_sources_summary.tsv; --write-sources: the records
// assigned to each source (kmc_classify_select, kmc_select_records -> source_<f>_<g>.fastq).
// GPU only: there is no CPU counting path here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <sys/stat.h>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "kmc.h"
#include "kmc_internal.h"
#include "kmc_stage.h"

namespace {

struct Options {
    std::string input;
    std::string out_dir = ".";
    std::string counts_path;
    int k = KMC_DROPIN_K;
    int dialect = 0;
    int64_t max_seqs = KMC_MAX_SEQS_REFERENCE;
    int gpus = 1;
    bool dropin = false;
    bool canonical = false;
    bool softmask = false;
    bool distances = true;
    bool canon_distances = false;
    bool quiet = false;
    bool host_loader = false;
    long sketch = 0;     // --sketch S: sketch size (0: none)
    long min_count = 1;  // --min-count C
    bool min_count_set = false;
    bool sketch_direct = false;  // --sketch-direct: kmc_sketch_from_sequences, no canonical count
    bool per_file = false;       // --per-file: one sketch per input file (kmc_sketch_from_sequences_grouped)
    bool max_seqs_set = false;
    std::string query;    // --query FILE: search FILE's sketches in the input's
    long top = 10;        // --top T: hits per query; 0: the whole rectangle
    long min_shared = 1;  // --min-shared M
    bool top_set = false, min_shared_set = false;
    std::vector<std::string> screen;  // --screen FILE (repeatable): the mixtures the inputs are looked for in
    std::vector<std::string> more_inputs;  // the input files after the first
    int format = 0;             // --format: 0 auto (by file name), 1 fasta, 2 fastq
    uint64_t screen_batch = 0;  // --screen-batch BYTES (0: the reader's default, 256 MiB)
    bool winner_takes_all = false;  // --winner-takes-all: with --screen, kmc_sketch_screen_winners' lines
    long min_abundance = 0;     // --min-abundance M: --per-file sketches of the k-mers seen M times (0: not given)
    long accum_slots = 0;       // --accum-slots LOG2 (0: the library's default)
    uint64_t batch = 0;         // --batch BYTES: the reader's batches of a --min-abundance FASTQ file
    bool accum_slots_set = false, batch_set = false;
    bool min_abundance_auto = false;  // --min-abundance auto: every file's M is its spectrum's valley
    long spectrum = 0;                // --spectrum B: the abundance spectrum of every input file, B bins (0: not given)
    double cluster = 0.0;  // --cluster D: clusters of the sketches at Mash distance D instead of their distances
    bool cluster_set = false;
    double pairs = 0.0;  // --pairs D: the list of the pairs within Mash distance D instead of every distance
    bool pairs_set = false;
    std::vector<std::string> recruit;  // --recruit FILE (repeatable): the reads matched against the inputs' k-mers
    long min_hits = 1;                 // --min-hits H: a listed record has at least H hits
    double min_fraction = 0.0;         // --min-fraction F: and hits >= F * sampled
    bool min_hits_set = false, min_fraction_set = false;
    bool write_recruited = false, write_rest = false;  // --write-recruited, --write-rest: the reads themselves
    bool classify = false;       // --classify: every input file is one source of the set's k-mers
    long min_margin = 1;         // --min-margin D: a record is assigned when source_hits - next_hits >= D
    bool min_margin_set = false;
    bool write_sources = false;  // --write-sources: the assigned reads themselves, per source
};

// auto: FASTQ exactly when the name ends in .fq or .fastq, whatever the case
bool is_fastq(const Options &o, const std::string &path) {
    if (o.format) return o.format == 2;
    for (const char *ext : {".fq", ".fastq"}) {
        const size_t n = strlen(ext);
        if (path.size() >= n && strcasecmp(path.c_str() + path.size() - n, ext) == 0) return true;
    }
    return false;
}

void usage(FILE *f) {
    fprintf(f,
            "usage: kmc [options] <input.fasta>\n"
            "       kmc --canonical --sketch S --sketch-direct --per-file [options] <a.fasta> <b.fasta> ...\n"
            "       kmc --canonical --sketch S --sketch-direct --query q.fasta [--top T] [options] <refs.fasta>\n"
            "       kmc --canonical --sketch S --sketch-direct --screen reads.fasta [--screen ...] [options] <refs.fasta>\n"
            "       kmc --canonical --sketch S --sketch-direct --screen reads.fastq [--screen-batch BYTES] [options] <refs.fasta>\n"
            "       kmc --canonical --sketch S --sketch-direct --screen reads.fasta --winner-takes-all [options] <refs.fasta>\n"
            "       kmc --canonical --sketch S --sketch-direct --per-file --min-abundance M [--batch BYTES] [options] <a.fastq> ...\n"
            "       kmc --canonical --sketch S --sketch-direct --per-file --spectrum B [--min-abundance auto] [options] <a.fastq> ...\n"
            "       kmc --canonical --sketch S [--sketch-direct] [--per-file] --cluster D [options] <input.fasta> ...\n"
            "       kmc --canonical --sketch S [--sketch-direct] [--per-file] --pairs D [--query q.fasta] [options] <input.fasta> ...\n"
            "       kmc -k K --canonical --recruit reads.fastq [--recruit more.fq] [--min-abundance M] [--min-hits H]\n"
            "           [--min-fraction F] --accum-slots L [--batch BYTES] [--write-recruited] [--write-rest] [options]\n"
            "       kmc -k K --canonical --recruit reads.fastq --classify [--min-margin D] [--write-sources]\n"
            "           --accum-slots L [recruit options] host.fa phage.fa ...\n"
            "           <host.fasta> <phage.fasta> ...\n"
            "       kmc synth OUT.fa RECORDS LENGTH [SEED]   (benchmark input, SURVEY.md 8(d))\n"
            "  -k K              k-mer length (default %d, the reference's K); dense path 1..%d,\n"
            "                    --canonical 1..%d\n"
            "  --dialect D       blank (importSeqs: records end at blank lines, default) or\n"
            "                    nonl (importSeqsNoNL: records also end at '>' headers)\n"
            "  --max-seqs N      the reference's MAX_SEQS cap (default %d, which keeps %d records\n"
            "                    like the reference); 0 = unlimited\n"
            "  --out DIR         directory of parallel_results.csv and sequential_results.csv\n"
            "                    (default .).  Both come from the GPU: without --dropin the two files\n"
            "                    hold the same vector (kmc_pair_distances, exact integer sums, which is\n"
            "                    what the reference's CPU sequentialKmerCount2 computes), so diffing them\n"
            "                    checks nothing; with --dropin parallel_results.csv holds minKmeres2_hip's\n"
            "                    float sums and sequential_results.csv the exact ones (no CPU path here)\n"
            "  --counts FILE     write the histogram: one line per k-mer code, 'kmer<TAB>c_0 .. c_n-1'\n"
            "                    (bin order of permutation(): first base least significant)\n"
            "  --no-distances    step 1 only (no step 2, no CSV)\n"
            "  --gpus N          count on N GPUs (records sharded, RCCL all-reduce)\n"
            "  --dropin          the exact reference launches: sumKmereCoincidencesGlobalMemory_hip\n"
            "                    and one minKmeres2_hip per record (k = %d, int32 offsets)\n"
            "  --canonical       canonical k-mers (k <= %d) instead of the dense histogram; with\n"
            "                    --counts writes 'record<TAB>kmer<TAB>count' lines\n"
            "  --distances       with --canonical: step 2 on the canonical counts\n"
            "                    (kmc_pair_distances_sparse), written to both CSVs in --out\n"
            "                    (without --canonical the dense path writes them anyway)\n"
            "  --sketch S        with --canonical: bottom-S MinHash sketch of every record's k-mers\n"
            "                    (kmc_sketch_from_counts, seed %llu, S in 1..%d) and the Mash distances\n"
            "                    of the sketches (kmc_sketch_distances), written to sketch_results.csv\n"
            "                    in --out; combines with --distances and --counts\n"
            "  --min-count C     with --canonical --sketch: only k-mers seen at least C times in their\n"
            "                    record are sketched (default 1: all)\n"
            "  --sketch-direct   with --canonical --sketch: sketch straight from the records\n"
            "                    (kmc_sketch_from_sequences: one pass, no canonical count, the same\n"
            "                    sketch_results.csv); not with --min-count above 1, --counts, --distances\n"
            "  --per-file        with --canonical --sketch S --sketch-direct: one or more input files,\n"
            "                    each sketched as one genome: the union of the k-mers of all its records\n"
            "                    (kmc_sketch_from_sequences_grouped); sketch_results.csv holds the distances\n"
            "                    between the files in command-line order, and one line per file gives its\n"
            "                    index, path, records and sketch size.  --max-seqs defaults to 0 here\n"
            "  --query FILE      with --canonical --sketch S --sketch-direct: the input file(s) are the\n"
            "                    references, sketched as without it (per record, or per file with\n"
            "                    --per-file); FILE is sketched the same way (per record, or as one genome\n"
            "                    with --per-file) and every query sketch is searched in the references\n"
            "                    (kmc_sketch_nearest).  <out>/query_results.tsv gets one line per hit:\n"
            "                    query<TAB>rank<TAB>ref<TAB>shared<TAB>denom<TAB>distance, rank from 1,\n"
            "                    best first; sketch_results.csv is not written\n"
            "  --top T           with --query: hits per query, 1..%d (default 10); 0: every query against\n"
            "                    every reference instead (kmc_sketch_distances_rect), written row-major,\n"
            "                    one distance per line, to <out>/query_distances.csv\n"
            "  --min-shared M    with --query: only references that share at least M sketch values with\n"
            "                    the query are hits (default 1; 0: unrelated references too, at distance 1)\n"
            "  --screen FILE     with --canonical --sketch S --sketch-direct, may be repeated, not with --query:\n"
            "                    the input file(s) are the references, sketched as without it (per record,\n"
            "                    or per file with --per-file); every FILE is a mixture (a read set, a\n"
            "                    metagenome) read whole (--max-seqs 0), and the hashes of ALL its k-mers are\n"
            "                    looked up among the references' sketch values (kmc_sketch_screen_build,\n"
            "                    _count once per FILE into one index, _results): containment, which a sketch\n"
            "                    of the mixture cannot give.  <out>/screen_results.tsv gets one line per\n"
            "                    reference, in reference order: index<TAB>shared<TAB>size<TAB>median<TAB>identity\n"
            "                    (shared: sketch values found; median: their median multiplicity; identity:\n"
            "                    (shared/size)^(1/k)), and <TAB>path with --per-file; sketch_results.csv is\n"
            "                    not written\n"
            "  --winner-takes-all with --screen only, for a redundant reference collection (Mash's screen -w):\n"
            "                    every found sketch value is credited to one reference only, the one with the\n"
            "                    largest shared/size that holds it, the earlier one on a tie\n"
            "                    (kmc_sketch_screen_winners).  The lines of screen_results.tsv are then\n"
            "                    index<TAB>won<TAB>size<TAB>median_won<TAB>identity_won<TAB>shared_all: the values\n"
            "                    won, their median multiplicity, (won/size)^(1/k), and in the extra column\n"
            "                    shared_all the `shared` of the plain screen; <TAB>path last with --per-file\n"
            "  --format F        auto (default), fasta or fastq, for every file of the command.  auto: a file\n"
            "                    whose name ends in .fq or .fastq (any case) is FASTQ, every other FASTA.\n"
            "                    FASTQ is strict four-line FASTQ (kmc_fastq_load_device: records are the\n"
            "                    sequence lines verbatim; --max-seqs N keeps the first N records; --dialect\n"
            "                    does not apply); a malformed file ends the run with its record index.\n"
            "                    Not with --host-loader, --gpus above 1 or --dropin\n"
            "  --screen-batch B  with --screen: a FASTQ FILE is streamed in batches of B raw bytes\n"
            "                    (kmc_fastq_open / _next / _close, one kmc_sketch_screen_count per batch), so it\n"
            "                    is never resident as a whole and may be a pipe (--format fastq --screen\n"
            "                    /dev/stdin); default 0: 256 MiB.  FASTA FILEs are read whole as before\n"
            "  --min-abundance M with --canonical --sketch S --sketch-direct --per-file only (the inputs, a --query\n"
            "                    FILE, the references of --screen): a file's sketch holds only the k-mers seen at\n"
            "                    least M times in the whole file, M >= 1 (Mash's -m; for read sets, whose k-mers\n"
            "                    seen once are mostly sequencing errors).  Every file is one pass of one\n"
            "                    accumulator (kmc_sketch_accum_*): a FASTQ file is streamed batch by batch\n"
            "                    (kmc_fastq_open / _next, one kmc_sketch_accum_add per batch), so it is never\n"
            "                    resident as a whole and may be a pipe (--format fastq /dev/stdin); a FASTA file\n"
            "                    is read whole and added in one call.  One line per file gives its records,\n"
            "                    batches, sketch size, threshold level j and whether the sketch is complete; a\n"
            "                    file whose sketch is not complete ends the run: raise --accum-slots\n"
            "                    M may be `auto`: every file then gets the min_abundance of its own abundance\n"
            "                    spectrum (kmc_spectrum_summarize: the valley between the k-mers of sequencing\n"
            "                    errors and the coverage peak; 1 for a file without one, such as an assembly),\n"
            "                    taken with the bins of --spectrum, or 256; its line then ends `min-abundance M`\n"
            "  --spectrum B      with --canonical --sketch S --sketch-direct --per-file only: the abundance spectrum\n"
            "                    of every input file (not of a --query FILE or the references of --screen), B bins\n"
            "                    in 2..%d: how many distinct k-mers the file holds once, twice, ... (the last bin:\n"
            "                    B - 1 times or more), taken from the accumulator's pass before its sketch\n"
            "                    (kmc_spectrum_from_accum); without --min-abundance that pass runs with M = 1, so\n"
            "                    the sketches are those of the run without --spectrum.  When the table holds only\n"
            "                    the k-mers whose hash is below a limit, the numbers are those of that uniform\n"
            "                    sample and scale = 2^64 / limit estimates the file's.  <out>/spectrum.tsv gets\n"
            "                    file<TAB>c<TAB>hist[c]<TAB>scale*hist[c] for every c >= 1 with hist[c] > 0;\n"
            "                    <out>/spectrum_summary.tsv one line per file: file, path, limit, scale, k-mers\n"
            "                    sampled, windows sampled, distinct, total, valley, peak, the M used, saturated,\n"
            "                    genome_size (kmc_spectrum_summarize)\n"
            "  --accum-slots L   with --min-abundance or --spectrum: the accumulator's table has 2^L slots, L in\n"
            "                    %d..%d (default 0: the power of two at or above %d S)\n"
            "  --batch B         with --min-abundance or --spectrum: raw bytes per batch of a streamed FASTQ file\n"
            "                    (default 0: 256 MiB)\n"
            "  --cluster D       with --canonical --sketch S (with or without --sketch-direct, --per-file,\n"
            "                    --min-count, --min-abundance), not with --query or --screen: the sketches,\n"
            "                    made as without it, are grouped at Mash distance D in 0..1 instead of\n"
            "                    compared (kmc_sketch_cluster at kmc_mash_jaccard_of_distance(D, k), single\n"
            "                    linkage: records whose distance is at most D, and everything such pairs\n"
            "                    connect, form a cluster).  <out>/clusters.tsv gets one line per record (per\n"
            "                    file with --per-file): index<TAB>representative<TAB>cluster<TAB>size, the\n"
            "                    representative being the cluster's smallest index and clusters numbered by\n"
            "                    it; sketch_results.csv is not written (no distance is kept)\n"
            "  --pairs D         with --canonical --sketch S (with or without --sketch-direct, --per-file,\n"
            "                    --min-count, --min-abundance), not with --cluster or --screen: only the pairs of\n"
            "                    sketches whose Mash distance is at most D in 0..1 are written, not every distance\n"
            "                    (kmc_sketch_links at kmc_mash_jaccard_of_distance(D, k): the pairs --cluster D\n"
            "                    links; Mash's dist -d).  <out>/pairs.tsv gets one line per pair i < j, sorted by\n"
            "                    (i, j): i<TAB>j<TAB>shared<TAB>denom<TAB>distance; sketch_results.csv is not\n"
            "                    written.  With --query FILE (and no --top): every query sketch against every\n"
            "                    reference sketch (kmc_sketch_links_rect), <out>/query_pairs.tsv with lines\n"
            "                    query<TAB>ref<TAB>shared<TAB>denom<TAB>distance sorted by (query, ref)\n"
            "  --recruit FILE    with --canonical and --accum-slots L (repeatable): all input files are added to one\n"
            "                    abundance accumulator of 2^L slots, the k-mer set (a FASTQ input batch by batch),\n"
            "                    and every record of FILE is matched against it (kmc_match_from_accum; a FASTQ\n"
            "                    FILE batch by batch, --batch).  <out>/read_matches.tsv gets, after a header line,\n"
            "                    one line file<TAB>record<TAB>windows<TAB>sampled<TAB>hits per listed record, in file\n"
            "                    order, then record order (record: 0-based within its file; windows: its valid\n"
            "                    k-mers; sampled: those below the set's hash limit, all of them when the table held\n"
            "                    every k-mer; hits: those in the set at least --min-abundance M times, default 1;\n"
            "                    auto is refused).  <out>/read_matches_summary.tsv gets, after a header line, one line\n"
            "                    per FILE: file, path, records, listed, limit, exact, sampled, hits.  A table that\n"
            "                    held only the k-mers below a hash limit is no error: they are a uniform sample and\n"
            "                    hits / sampled estimates the fraction; `exact` and `limit` say so.  Not with --sketch,\n"
            "                    --screen, --query, --cluster, --pairs, --distances or --spectrum\n"
            "  --min-hits H      with --recruit: a record is listed when hits >= H (default 1)\n"
            "  --min-fraction F  with --recruit: and hits >= F * sampled, F in 0..1 (default 0)\n"
            "  --write-recruited with --recruit, every FILE in FASTQ: <out>/recruited_<f>.fastq (f: the file's number\n"
            "                    in read_matches.tsv) gets the listed records of FILE as the raw bytes of the input,\n"
            "                    headers, qualities and line ends included, in input order (kmc_match_select,\n"
            "                    kmc_select_records on each batch's raw text, then device to file)\n"
            "  --write-rest      the same for the records that are not listed: <out>/rest_<f>.fastq (depletion).\n"
            "                    Either option holds one more raw batch of device memory (--batch), shared by both\n"
            "  --classify        with --recruit: every input file is one source, in command-line order (32 at most,\n"
            "                    regular files: they are read twice).  After all adds the inputs are read again and\n"
            "                    the set's k-mers labelled with the sources that hold them (kmc_label_accum);\n"
            "                    per batch kmc_classify_from_accum replaces the match.  <out>/read_sources.tsv gets,\n"
            "                    after a header line, the lines of read_matches.tsv with three more columns: source\n"
            "                    (the source with the most hits, the smaller number on a tie, - for none),\n"
            "                    source_hits (the hits that source holds) and next_hits (the most any other source\n"
            "                    holds).  <out>/read_sources_summary.tsv gets, after a header line, per FILE one line\n"
            "                    file, source, path, best, assigned per source (best: the listed records with that\n"
            "                    source; assigned: those of them with source_hits - next_hits >= D) and one line\n"
            "                    with source - and path - (best: the listed records with no source; assigned: the\n"
            "                    listed records assigned to none).  The other outputs are as without --classify\n"
            "  --min-margin D    with --classify: D in 0..4294967295, default 1: a tie is assigned to nobody\n"
            "  --write-sources   with --classify, every FILE in FASTQ: <out>/source_<f>_<g>.fastq gets the records of\n"
            "                    FILE assigned to source g as the raw bytes of the input, in input order\n"
            "                    (kmc_classify_select, kmc_select_records)\n"
            "  --softmask        with --canonical: lowercase acgt count as bases\n"
            "  --host-loader     parse the FASTA on the host (kmc_fasta_load) instead of on the GPU\n"
            "                    (kmc_fasta_load_device); --gpus > 1 always uses the host buffer\n"
            "  -q                quiet (no progress lines)\n",
            KMC_DROPIN_K, KMC_DENSE_MAX_K, KMC_CANON_MAX_K, KMC_MAX_SEQS_REFERENCE, KMC_MAX_SEQS_REFERENCE + 1,
            KMC_DROPIN_K, KMC_CANON_MAX_K, (unsigned long long)KMC_SKETCH_DEFAULT_SEED, KMC_SKETCH_MAX_SIZE,
            KMC_NEAREST_MAX_TOP, KMC_SPECTRUM_MAX_BINS, KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS, KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS,
            KMC_SKETCH_ACCUM_DEFAULT_SLOTS_PER_VALUE);
}

int parse(int argc, char **argv, Options &o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&](const char *what) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "kmc: %s needs a value\n", what);
                exit(2);
            }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            usage(stdout);
            exit(0);
        } else if (a == "-k") {
            o.k = atoi(next("-k"));
        } else if (a == "--dialect") {
            const std::string d = next("--dialect");
            if (d == "blank") o.dialect = 0;
            else if (d == "nonl") o.dialect = 1;
            else return fprintf(stderr, "kmc: unknown dialect '%s'\n", d.c_str()), 2;
        } else if (a == "--max-seqs") {
            o.max_seqs = atoll(next("--max-seqs"));
            o.max_seqs_set = true;
        } else if (a == "--out") {
            o.out_dir = next("--out");
        } else if (a == "--counts") {
            o.counts_path = next("--counts");
        } else if (a == "--no-distances") {
            o.distances = false;
        } else if (a == "--distances") {
            o.canon_distances = true;
        } else if (a == "--gpus") {
            o.gpus = atoi(next("--gpus"));
        } else if (a == "--dropin") {
            o.dropin = true;
        } else if (a == "--canonical") {
            o.canonical = true;
        } else if (a == "--sketch") {
            o.sketch = atol(next("--sketch"));
            if (o.sketch < 1 || o.sketch > KMC_SKETCH_MAX_SIZE)
                return fprintf(stderr, "kmc: --sketch must be in 1..%d\n", KMC_SKETCH_MAX_SIZE), 2;
        } else if (a == "--sketch-direct") {
            o.sketch_direct = true;
        } else if (a == "--per-file") {
            o.per_file = true;
        } else if (a == "--min-count") {
            o.min_count = atol(next("--min-count"));
            o.min_count_set = true;
            if (o.min_count < 0 || o.min_count > (long)UINT32_MAX)
                return fprintf(stderr, "kmc: --min-count out of range\n"), 2;
        } else if (a == "--query") {
            o.query = next("--query");
        } else if (a == "--screen") {
            o.screen.push_back(next("--screen"));
        } else if (a == "--winner-takes-all") {
            o.winner_takes_all = true;
        } else if (a == "--top") {
            o.top = atol(next("--top"));
            o.top_set = true;
        } else if (a == "--min-shared") {
            o.min_shared = atol(next("--min-shared"));
            o.min_shared_set = true;
        } else if (a == "--format") {
            const std::string f = next("--format");
            if (f == "auto") o.format = 0;
            else if (f == "fasta") o.format = 1;
            else if (f == "fastq") o.format = 2;
            else return fprintf(stderr, "kmc: unknown format '%s' (auto, fasta, fastq)\n", f.c_str()), 2;
        } else if (a == "--screen-batch") {
            const long long b = atoll(next("--screen-batch"));
            if (b < 0 || b >= (1ll << 32)) return fprintf(stderr, "kmc: --screen-batch must be in 0..2^32-1\n"), 2;
            o.screen_batch = (uint64_t)b;
        } else if (a == "--min-abundance") {
            const char *v = next("--min-abundance");
            o.min_abundance_auto = strcmp(v, "auto") == 0;
            o.min_abundance = o.min_abundance_auto ? 1 : atol(v);
            if (o.min_abundance < 1 || o.min_abundance > (long)UINT32_MAX) {
                fprintf(stderr, "kmc: --min-abundance must be in 1..%u, or auto\n", UINT32_MAX);
                return usage(stderr), 2;
            }
        } else if (a == "--spectrum") {
            o.spectrum = atol(next("--spectrum"));
            if (o.spectrum < 2 || o.spectrum > KMC_SPECTRUM_MAX_BINS) {
                fprintf(stderr, "kmc: --spectrum must be in 2..%d\n", KMC_SPECTRUM_MAX_BINS);
                return usage(stderr), 2;
            }
        } else if (a == "--accum-slots") {
            o.accum_slots = atol(next("--accum-slots"));
            o.accum_slots_set = true;
            if (o.accum_slots != 0 && (o.accum_slots < KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS ||
                                       o.accum_slots > KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS)) {
                fprintf(stderr, "kmc: --accum-slots must be 0 or in %d..%d\n", KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS,
                        KMC_SKETCH_ACCUM_MAX_LOG2_SLOTS);
                return usage(stderr), 2;
            }
        } else if (a == "--batch") {
            const long long b = atoll(next("--batch"));
            o.batch_set = true;
            if (b < 0 || b >= (1ll << 32)) {
                fprintf(stderr, "kmc: --batch must be in 0..2^32-1\n");
                return usage(stderr), 2;
            }
            o.batch = (uint64_t)b;
        } else if (a == "--cluster") {
            char *end = nullptr;
            const char *v = next("--cluster");
            o.cluster = strtod(v, &end);
            o.cluster_set = true;
            if (end == v || *end != '\0' || !(o.cluster >= 0.0 && o.cluster <= 1.0)) {
                fprintf(stderr, "kmc: --cluster takes a Mash distance in 0..1\n");
                return usage(stderr), 2;
            }
        } else if (a == "--pairs") {
            char *end = nullptr;
            const char *v = next("--pairs");
            o.pairs = strtod(v, &end);
            o.pairs_set = true;
            if (end == v || *end != '\0' || !(o.pairs >= 0.0 && o.pairs <= 1.0)) {
                fprintf(stderr, "kmc: --pairs takes a Mash distance in 0..1\n");
                return usage(stderr), 2;
            }
        } else if (a == "--recruit") {
            o.recruit.push_back(next("--recruit"));
        } else if (a == "--min-hits") {
            char *end = nullptr;
            const char *v = next("--min-hits");
            o.min_hits = strtol(v, &end, 10);
            o.min_hits_set = true;
            if (end == v || *end != '\0' || o.min_hits < 0 || o.min_hits > (long)UINT32_MAX) {
                fprintf(stderr, "kmc: --min-hits must be in 0..%u\n", UINT32_MAX);
                return usage(stderr), 2;
            }
        } else if (a == "--min-fraction") {
            char *end = nullptr;
            const char *v = next("--min-fraction");
            o.min_fraction = strtod(v, &end);
            o.min_fraction_set = true;
            if (end == v || *end != '\0' || !(o.min_fraction >= 0.0 && o.min_fraction <= 1.0)) {
                fprintf(stderr, "kmc: --min-fraction takes a fraction in 0..1\n");
                return usage(stderr), 2;
            }
        } else if (a == "--write-recruited") {
            o.write_recruited = true;
        } else if (a == "--write-rest") {
            o.write_rest = true;
        } else if (a == "--classify") {
            o.classify = true;
        } else if (a == "--write-sources") {
            o.write_sources = true;
        } else if (a == "--min-margin") {
            char *end = nullptr;
            const char *v = next("--min-margin");
            o.min_margin = strtol(v, &end, 10);
            o.min_margin_set = true;
            if (end == v || *end != '\0' || o.min_margin < 0 || o.min_margin > (long)UINT32_MAX) {
                fprintf(stderr, "kmc: --min-margin must be in 0..%u\n", UINT32_MAX);
                return usage(stderr), 2;
            }
        } else if (a == "--softmask") {
            o.softmask = true;
        } else if (a == "--host-loader") {
            o.host_loader = true;
        } else if (a == "-q") {
            o.quiet = true;
        } else if (!a.empty() && a[0] == '-') {
            return fprintf(stderr, "kmc: unknown option '%s'\n", a.c_str()), 2;
        } else if (o.input.empty()) {
            o.input = a;
        } else {
            o.more_inputs.push_back(a);
        }
    }
    if (o.input.empty()) return usage(stderr), 2;
    if (!o.more_inputs.empty() && !o.per_file && o.recruit.empty()) return fprintf(stderr, "kmc: more than one input file\n"), 2;
    if (o.dropin && o.k != KMC_DROPIN_K)
        return fprintf(stderr, "kmc: --dropin is the k = %d reference launch\n", KMC_DROPIN_K), 2;
    if (o.canonical ? (o.k < 1 || o.k > KMC_CANON_MAX_K) : (o.k < 1 || o.k > KMC_DENSE_MAX_K))
        return fprintf(stderr, "kmc: k = %d out of range\n", o.k), 2;
    if ((o.min_hits_set || o.min_fraction_set) && o.recruit.empty()) {
        fprintf(stderr, "kmc: --min-hits and --min-fraction select the lines of --recruit\n");
        return usage(stderr), 2;
    }
    if ((o.write_recruited || o.write_rest) && o.recruit.empty()) {
        fprintf(stderr, "kmc: --write-recruited and --write-rest write the reads of --recruit\n");
        return usage(stderr), 2;
    }
    if ((o.classify || o.min_margin_set || o.write_sources) && o.recruit.empty()) {
        fprintf(stderr, "kmc: --classify, --min-margin and --write-sources tell the reads of --recruit apart\n");
        return usage(stderr), 2;
    }
    if ((o.min_margin_set || o.write_sources) && !o.classify) {
        fprintf(stderr, "kmc: --min-margin and --write-sources need --classify\n");
        return usage(stderr), 2;
    }
    if (!o.recruit.empty()) {
        if (!o.canonical) {
            fprintf(stderr, "kmc: --recruit needs --canonical\n");
            return usage(stderr), 2;
        }
        if (o.sketch > 0 || !o.screen.empty() || !o.query.empty() || o.cluster_set || o.pairs_set || o.canon_distances ||
            o.spectrum > 0) {
            fprintf(stderr, "kmc: --recruit matches reads against the k-mers of the input files: not with --sketch, "
                            "--screen, --query, --cluster, --pairs, --distances or --spectrum\n");
            return usage(stderr), 2;
        }
        if (o.min_abundance_auto) {
            fprintf(stderr, "kmc: --recruit takes the count a k-mer needs as --min-abundance M: not --min-abundance auto\n");
            return usage(stderr), 2;
        }
        if (!o.accum_slots_set || o.accum_slots == 0) {
            fprintf(stderr, "kmc: --recruit needs --accum-slots L, the size of the k-mer set's table\n");
            return usage(stderr), 2;
        }
        if (o.max_seqs_set && o.max_seqs > 0) {
            fprintf(stderr, "kmc: --recruit reads every file whole: not with --max-seqs above 0\n");
            return usage(stderr), 2;
        }
        o.max_seqs = 0;
        if (o.write_recruited || o.write_rest)
            for (const std::string &f : o.recruit)
                if (!is_fastq(o, f)) {
                    fprintf(stderr, "kmc: --write-recruited and --write-rest write FASTQ records: %s is not FASTQ "
                                    "(--format, or a .fq / .fastq name)\n", f.c_str());
                    return usage(stderr), 2;
                }
        if (o.write_sources)
            for (const std::string &f : o.recruit)
                if (!is_fastq(o, f)) {
                    fprintf(stderr, "kmc: --write-sources writes FASTQ records: %s is not FASTQ (--format, or a .fq / "
                                    ".fastq name)\n", f.c_str());
                    return usage(stderr), 2;
                }
        if (o.classify) {
            if (1 + o.more_inputs.size() > KMC_CLASSIFY_MAX_SOURCES) {
                fprintf(stderr, "kmc: --classify tells %d sources apart at most: %zu input files\n",
                        KMC_CLASSIFY_MAX_SOURCES, 1 + o.more_inputs.size());
                return usage(stderr), 2;
            }
            // the inputs are read twice (add, then label): nothing is read from one that cannot be
            std::vector<std::string> inputs{o.input};
            inputs.insert(inputs.end(), o.more_inputs.begin(), o.more_inputs.end());
            for (const std::string &f : inputs) {
                struct stat sb;
                if (stat(f.c_str(), &sb) == 0 && !S_ISREG(sb.st_mode)) {
                    fprintf(stderr, "kmc: --classify reads every input file twice: %s is not a regular file\n", f.c_str());
                    return 2;
                }
            }
        }
    }
    if ((o.sketch > 0 || o.min_count_set) && !o.canonical) {
        fprintf(stderr, "kmc: --sketch and --min-count need --canonical\n");
        return usage(stderr), 2;
    }
    if (o.min_count_set && o.sketch == 0) {
        fprintf(stderr, "kmc: --min-count filters what --sketch takes\n");
        return usage(stderr), 2;
    }
    if (o.sketch_direct && !(o.canonical && o.sketch > 0)) {
        fprintf(stderr, "kmc: --sketch-direct needs --canonical --sketch S\n");
        return usage(stderr), 2;
    }
    if (o.sketch_direct && (o.min_count > 1 || !o.counts_path.empty() || o.canon_distances)) {
        fprintf(stderr, "kmc: --sketch-direct never counts: not with --min-count above 1, --counts or --distances\n");
        return usage(stderr), 2;
    }
    if (o.per_file && !(o.canonical && o.sketch > 0 && o.sketch_direct)) {
        fprintf(stderr, "kmc: --per-file needs --canonical --sketch S --sketch-direct\n");
        return usage(stderr), 2;
    }
    if (o.min_abundance > 0 && !o.per_file && o.recruit.empty()) {
        fprintf(stderr, "kmc: --min-abundance needs --canonical --sketch S --sketch-direct --per-file\n");
        return usage(stderr), 2;
    }
    if (o.min_abundance > 0 && o.max_seqs_set && o.max_seqs > 0) {
        fprintf(stderr, "kmc: --min-abundance reads every file whole: not with --max-seqs above 0\n");
        return usage(stderr), 2;
    }
    if (o.spectrum > 0 && !o.per_file) {
        fprintf(stderr, "kmc: --spectrum needs --canonical --sketch S --sketch-direct --per-file\n");
        return usage(stderr), 2;
    }
    if (o.spectrum > 0 && o.max_seqs_set && o.max_seqs > 0) {
        fprintf(stderr, "kmc: --spectrum reads every file whole: not with --max-seqs above 0\n");
        return usage(stderr), 2;
    }
    if ((o.accum_slots_set || o.batch_set) && o.min_abundance == 0 && o.spectrum == 0 && o.recruit.empty()) {
        fprintf(stderr, "kmc: --accum-slots and --batch shape the pass of --min-abundance or --spectrum\n");
        return usage(stderr), 2;
    }
    if (o.spectrum > 0 && o.min_abundance == 0) o.min_abundance = 1;  // the accumulator's pass, every k-mer
    if (o.per_file && !o.max_seqs_set) o.max_seqs = 0;
    if (!o.query.empty() && !(o.canonical && o.sketch > 0 && o.sketch_direct)) {
        fprintf(stderr, "kmc: --query needs --canonical --sketch S --sketch-direct\n");
        return usage(stderr), 2;
    }
    if (!o.screen.empty() && !(o.canonical && o.sketch > 0 && o.sketch_direct)) {
        fprintf(stderr, "kmc: --screen needs --canonical --sketch S --sketch-direct\n");
        return usage(stderr), 2;
    }
    if (!o.screen.empty() && !o.query.empty()) {
        fprintf(stderr, "kmc: --screen and --query exclude each other\n");
        return usage(stderr), 2;
    }
    if (o.winner_takes_all && o.screen.empty()) {
        fprintf(stderr, "kmc: --winner-takes-all credits the values of --screen\n");
        return usage(stderr), 2;
    }
    if ((o.top_set || o.min_shared_set) && o.query.empty()) {
        fprintf(stderr, "kmc: --top and --min-shared select the hits of --query\n");
        return usage(stderr), 2;
    }
    if (o.top < 0 || o.top > KMC_NEAREST_MAX_TOP || o.min_shared < 0 || o.min_shared > (long)UINT32_MAX) {
        fprintf(stderr, "kmc: --top must be in 0..%d, --min-shared in 0..%u\n", KMC_NEAREST_MAX_TOP, UINT32_MAX);
        return usage(stderr), 2;
    }
    if (o.cluster_set && (o.sketch == 0 || !o.query.empty() || !o.screen.empty())) {
        fprintf(stderr, "kmc: --cluster groups the sketches of --canonical --sketch S: not with --query or --screen\n");
        return usage(stderr), 2;
    }
    if (o.pairs_set && o.sketch == 0) {
        fprintf(stderr, "kmc: --pairs lists the pairs of the sketches of --canonical --sketch S\n");
        return usage(stderr), 2;
    }
    if (o.pairs_set && o.cluster_set) {
        fprintf(stderr, "kmc: --pairs and --cluster exclude each other\n");
        return usage(stderr), 2;
    }
    if (o.pairs_set && !o.screen.empty()) {
        fprintf(stderr, "kmc: --pairs and --screen exclude each other\n");
        return usage(stderr), 2;
    }
    if (o.pairs_set && o.top_set) {
        fprintf(stderr, "kmc: --pairs lists every pair of --query within its distance: not with --top\n");
        return usage(stderr), 2;
    }
    if (o.screen_batch && o.screen.empty()) {
        fprintf(stderr, "kmc: --screen-batch sets the batches of --screen\n");
        return usage(stderr), 2;
    }
    if (o.gpus < 1) return fprintf(stderr, "kmc: --gpus must be >= 1\n"), 2;
    if (o.host_loader || o.gpus > 1 || o.dropin) {  // the paths that need the host FASTA loader's buffer
        std::vector<std::string> files{o.input};
        files.insert(files.end(), o.more_inputs.begin(), o.more_inputs.end());
        files.insert(files.end(), o.screen.begin(), o.screen.end());
        files.insert(files.end(), o.recruit.begin(), o.recruit.end());
        if (!o.query.empty()) files.push_back(o.query);
        for (const std::string &f : files)
            if (is_fastq(o, f))
                return fprintf(stderr, "kmc: %s: FASTQ input is not read with --host-loader, --gpus above 1 or --dropin\n",
                               f.c_str()), 2;
    }
    if (o.gpus > 1 && (o.dropin || o.canonical))
        return fprintf(stderr, "kmc: --gpus > 1 is for the dense path\n"), 2;
    return 0;
}

#define HIPCHK(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "kmc: %s failed: %s\n", #x, hipGetErrorString(e_));                    \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

#define KMCCHK(x)                                                                                  \
    do {                                                                                           \
        int rc_ = (x);                                                                             \
        if (rc_ != 0) {                                                                            \
            fprintf(stderr, "kmc: %s failed: %d (%s)\n", #x, rc_, kmc_error_string(rc_));          \
            return 1;                                                                              \
        }                                                                                          \
    } while (0)

// k-mer text of a dense code (first base = least significant 2 bits)
std::string dense_kmer(uint64_t code, int k) {
    std::string s(k, 'A');
    for (int p = 0; p < k; ++p) s[p] = "ACGT"[(code >> (2 * p)) & 3];
    return s;
}

// k-mer text of a canonical key (first base = most significant 2 bits)
std::string canon_kmer(uint64_t key, int k) {
    std::string s(k, 'A');
    for (int p = 0; p < k; ++p) s[p] = "ACGT"[(key >> (2 * (k - 1 - p))) & 3];
    return s;
}

int write_counts(const std::string &path, const std::vector<int32_t> &sum, uint64_t n, int k) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    const uint64_t nb = 1ull << (2 * k);
    std::string line;
    for (uint64_t c = 0; c < nb; ++c) {
        line = dense_kmer(c, k);
        char buf[16];
        for (uint64_t s = 0; s < n; ++s) {
            snprintf(buf, sizeof buf, "\t%d", sum[s + n * c]);
            line += buf;
        }
        line += '\n';
        fwrite(line.data(), 1, line.size(), f);
    }
    return fclose(f) == 0 ? 0 : 1;
}

int write_csv(const std::string &path, const std::vector<float> &d) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    for (float v : d) fprintf(f, "%f\n", v);  // main.cu:357
    return fclose(f) == 0 ? 0 : 1;
}

float ms_between(hipEvent_t a, hipEvent_t b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.f;
    return ms;
}

// Move-only owners: every path out of run(), failing or not, releases what it acquired.
// A release's own error is ignored: it must not turn a finished run into a failure.
struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FastaFree { void operator()(kmc_fasta *f) const { kmc_fasta_free(f); } };
struct FastqClose { void operator()(kmc_fastq_reader *r) const { kmc_fastq_close(r); } };
struct AccumFree { void operator()(kmc_sketch_accum *a) const { kmc_sketch_accum_free(a); } };
struct FileClose { void operator()(FILE *f) const { (void)fclose(f); } };
template <class T>
using DevBuf = std::unique_ptr<T, DevFree>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Fasta = std::unique_ptr<kmc_fasta, FastaFree>;
using FastqReader = std::unique_ptr<kmc_fastq_reader, FastqClose>;
using Accum = std::unique_ptr<kmc_sketch_accum, AccumFree>;
using File = std::unique_ptr<FILE, FileClose>;

// a file descriptor that is closed with its owner (-1: none)
class Fd {
public:
    Fd() = default;
    Fd(const Fd &) = delete;
    Fd &operator=(const Fd &) = delete;
    ~Fd() { reset(-1); }
    int get() const { return fd_; }
    void reset(int fd) {
        if (fd_ >= 0) (void)close(fd_);
        fd_ = fd;
    }
    int release() {
        const int fd = fd_;
        fd_ = -1;
        return fd;
    }

private:
    int fd_ = -1;
};

// max(count, 1) elements: an empty input still gets a pointer the entry points take
template <class T>
hipError_t dev_alloc(DevBuf<T> &b, uint64_t count) {
    T *p = nullptr;
    const hipError_t e = hipMalloc(&p, std::max<uint64_t>(count, 1) * sizeof(T));
    b.reset(p);
    return e;
}

// null where it cannot be created: the hipEventRecord that follows reports that
Event make_event() {
    hipEvent_t e = nullptr;
    return Event(hipEventCreate(&e) == hipSuccess ? e : nullptr);
}

// the record buffer, resident on device 0 for steps 1 and 2
struct Records {
    Fasta fa;  // the host loader's copy (kmc_count_multi reads it); none after the GPU parse
    DevBuf<char> data;
    DevBuf<int64_t> idx;
    std::vector<int64_t> hidx;
    uint64_t n = 0, bytes = 0;
};

int malformed(const std::string &path, uint64_t record) {
    return fprintf(stderr, "kmc: %s: malformed FASTQ at record %" PRIu64 "\n", path.c_str(), record), 1;
}

// parsed on the GPU from the raw file bytes (FASTA or FASTQ), or FASTA parsed on the host and copied
int load(const Options &o, hipStream_t st, Records &r) {
    const bool host = o.host_loader || o.gpus > 1;
    const auto tl0 = std::chrono::steady_clock::now();
    if (is_fastq(o, o.input)) {
        char *d_data = nullptr;
        int64_t *d_idx = nullptr;
        const int rc = kmc_fastq_load_device(o.input.c_str(), o.max_seqs, &d_data, &r.bytes, &d_idx, &r.n, st);
        if (rc == KMC_ERR_FORMAT) return malformed(o.input, r.n);
        KMCCHK(rc);
        r.data.reset(d_data);
        r.idx.reset(d_idx);
        r.hidx.resize(r.n + 1);
        HIPCHK(hipMemcpy(r.hidx.data(), d_idx, (r.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    } else if (host) {
        kmc_fasta *fa = nullptr;
        KMCCHK(kmc_fasta_load(o.input.c_str(), o.dialect, o.max_seqs, &fa));
        r.fa.reset(fa);
        r.n = kmc_fasta_num_seqs(fa);
        r.bytes = kmc_fasta_data_bytes(fa);
        r.hidx.assign(kmc_fasta_indices(fa), kmc_fasta_indices(fa) + r.n + 1);
        HIPCHK(dev_alloc(r.data, r.bytes + 16));
        HIPCHK(dev_alloc(r.idx, r.n + 1));
        if (r.bytes) HIPCHK(hipMemcpyAsync(r.data.get(), kmc_fasta_data(fa), r.bytes, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(r.idx.get(), r.hidx.data(), (r.n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    } else {
        char *d_data = nullptr;
        int64_t *d_idx = nullptr;
        KMCCHK(kmc_fasta_load_device(o.input.c_str(), o.dialect, o.max_seqs, &d_data, &r.bytes, &d_idx, &r.n, st));
        r.data.reset(d_data);
        r.idx.reset(d_idx);
        r.hidx.resize(r.n + 1);
        HIPCHK(hipMemcpy(r.hidx.data(), d_idx, (r.n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    }
    const auto tl1 = std::chrono::steady_clock::now();
    if (!o.quiet) {
        printf("K = %d\n", o.k);
        printf("Size all seqs:%" PRIu64 "\n", r.bytes);  // main.cu:166-167
        printf("%" PRIu64 " sequences read .\n", r.n);
        printf("Load (%s parse, file to device): %.1f ms\n", host ? "host" : "GPU",
               std::chrono::duration<double, std::milli>(tl1 - tl0).count());
    }
    return 0;
}

// Step 2 of every mode: `enqueue` puts the n(n-1)/2 distances (a device vector) on st and
// returns its status; `out` gets them.  Unless -q, `report` prints the mode's timer lines
// from the events around that work.  Without a pair nothing runs or prints, unless `even_empty`.
template <class Enqueue, class Report>
int step2(const Options &o, uint64_t n, hipStream_t st, bool even_empty, std::vector<float> &out, Enqueue enqueue,
          Report report) {
    const uint64_t npairs = n * (n > 0 ? n - 1 : 0) / 2;
    out.assign(npairs, 0.f);
    if (npairs == 0 && !even_empty) return 0;
    DevBuf<float> d_out;
    Event t0 = make_event(), t1 = make_event();
    HIPCHK(dev_alloc(d_out, npairs));
    HIPCHK(hipEventRecord(t0.get(), st));
    KMCCHK(enqueue(d_out.get()));
    HIPCHK(hipEventRecord(t1.get(), st));
    HIPCHK(hipEventSynchronize(t1.get()));
    if (!o.quiet) report(t0.get(), t1.get());
    if (npairs > 0) HIPCHK(hipMemcpy(out.data(), d_out.get(), npairs * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// --cluster D: the rows' clusters at Mash distance D, clusters.tsv; no distance leaves the device
int cluster_step(const Options &o, const uint64_t *d_sk, const uint32_t *d_sz, uint64_t n, hipStream_t st,
                 hipEvent_t r0, hipEvent_t r1) {
    const uint32_t s = (uint32_t)o.sketch;
    DevBuf<uint32_t> d_lab, d_idx;
    Event t0 = make_event(), t1 = make_event();
    HIPCHK(dev_alloc(d_lab, n));
    HIPCHK(dev_alloc(d_idx, n));
    HIPCHK(hipEventRecord(t0.get(), st));
    KMCCHK(kmc_sketch_cluster(d_sk, d_sz, n, s, kmc_mash_jaccard_of_distance(o.cluster, o.k), d_lab.get(), d_idx.get(),
                              nullptr, nullptr, 0, st));
    HIPCHK(hipEventRecord(t1.get(), st));
    HIPCHK(hipEventSynchronize(t1.get()));
    std::vector<uint32_t> lab(n), idx(n), size(n, 0);
    if (n > 0) {
        HIPCHK(hipMemcpy(lab.data(), d_lab.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(idx.data(), d_idx.get(), n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    uint64_t clusters = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (lab[i] >= n) return fprintf(stderr, "kmc: kmc_sketch_cluster: label out of range\n"), 1;
        clusters += size[lab[i]]++ == 0;
    }
    if (!o.quiet) {
        printf("Sketch (s=%u): %.3f ms\n", s, ms_between(r0, r1));
        printf("Sketch clusters (distance <= %g): %.3f ms, %" PRIu64 " clusters of %" PRIu64 " records\n", o.cluster,
               ms_between(t0.get(), t1.get()), clusters, n);
    }
    const std::string path = o.out_dir + "/clusters.tsv";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    for (uint64_t i = 0; i < n; ++i) fprintf(f, "%" PRIu64 "\t%u\t%u\t%u\n", i, lab[i], idx[i], size[lab[i]]);
    return fclose(f) == 0 ? 0 : 1;
}

// --pairs D: the pairs within Mash distance D with their counts and distances, sorted, as
// `name` in --out: the pairs i < j of the rows R (Q null: kmc_sketch_links), or every query
// row of Q against every row of R (kmc_sketch_links_rect).  One call with room for
// min(all pairs, 2^26) entries; a second one of exactly *num_links when they did not fit.
int pairs_step(const Options &o, const uint64_t *q_sk, const uint32_t *q_sz, uint64_t m, const uint64_t *r_sk,
               const uint32_t *r_sz, uint64_t n, hipStream_t st, const char *name) {
    const uint32_t s = (uint32_t)o.sketch;
    const double min_jaccard = kmc_mash_jaccard_of_distance(o.pairs, o.k);
    const uint64_t all = q_sk ? m * n : n * (n > 0 ? n - 1 : 0) / 2;
    uint64_t capacity = std::min<uint64_t>(all, 1ull << 26), found = 0;
    DevBuf<kmc_sketch_link> d_links;
    DevBuf<float> d_dist;
    DevBuf<uint64_t> d_count;
    Event t0 = make_event(), t1 = make_event();
    HIPCHK(dev_alloc(d_count, 1));
    HIPCHK(hipEventRecord(t0.get(), st));
    for (int call = 0; call < 2; ++call) {
        HIPCHK(dev_alloc(d_links, capacity));
        HIPCHK(dev_alloc(d_dist, capacity));
        if (q_sk)
            KMCCHK(kmc_sketch_links_rect(q_sk, q_sz, m, r_sk, r_sz, n, s, o.k, min_jaccard, d_links.get(), d_dist.get(),
                                         capacity, d_count.get(), st));
        else
            KMCCHK(kmc_sketch_links(r_sk, r_sz, n, s, o.k, min_jaccard, d_links.get(), d_dist.get(), capacity,
                                    d_count.get(), st));
        HIPCHK(hipMemcpyAsync(&found, d_count.get(), sizeof found, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (found <= capacity) break;
        if (call == 1) return fprintf(stderr, "kmc: kmc_sketch_links: the list grew between two calls\n"), 1;
        capacity = found;
    }
    HIPCHK(hipEventRecord(t1.get(), st));
    HIPCHK(hipEventSynchronize(t1.get()));
    std::vector<kmc_sketch_link> links(found);
    std::vector<float> dist(found);
    if (found > 0) {
        HIPCHK(hipMemcpy(links.data(), d_links.get(), found * sizeof(kmc_sketch_link), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist.data(), d_dist.get(), found * sizeof(float), hipMemcpyDeviceToHost));
    }
    std::vector<uint64_t> order(found);  // the entries by (i, j): the device's order is unspecified
    for (uint64_t e = 0; e < found; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        return links[a].i != links[b].i ? links[a].i < links[b].i : links[a].j < links[b].j;
    });
    if (!o.quiet) {
        printf("Sketch pairs (distance <= %g): %.3f ms\n", o.pairs, ms_between(t0.get(), t1.get()));
        if (q_sk)
            printf("%" PRIu64 " pairs within %g of %" PRIu64 " queries and %" PRIu64 " records\n", found, o.pairs, m, n);
        else
            printf("%" PRIu64 " pairs within %g of %" PRIu64 " records\n", found, o.pairs, n);
    }
    const std::string path = o.out_dir + "/" + name;
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    for (uint64_t e : order)
        fprintf(f, "%u\t%u\t%u\t%u\t%f\n", links[e].i, links[e].j, links[e].shared, links[e].denom, dist[e]);
    return fclose(f) == 0 ? 0 : 1;
}

// --sketch: the rows of every record (make_rows: from the canonical lists or, with
// --sketch-direct, from the record buffer), their Mash distances, sketch_results.csv
template <class MakeRows>
int sketch_step(const Options &o, MakeRows make_rows, uint64_t n, hipStream_t st) {
    const uint32_t s = (uint32_t)o.sketch;
    DevBuf<uint64_t> d_sk;
    DevBuf<uint32_t> d_sz;
    Event r0 = make_event(), r1 = make_event();
    HIPCHK(dev_alloc(d_sk, n * s));
    HIPCHK(dev_alloc(d_sz, n));
    HIPCHK(hipEventRecord(r0.get(), st));
    KMCCHK(make_rows(s, d_sk.get(), d_sz.get()));
    HIPCHK(hipEventRecord(r1.get(), st));
    if (o.cluster_set) return cluster_step(o, d_sk.get(), d_sz.get(), n, st, r0.get(), r1.get());
    if (o.pairs_set) {
        HIPCHK(hipEventSynchronize(r1.get()));
        if (!o.quiet) printf("Sketch (s=%u): %.3f ms\n", s, ms_between(r0.get(), r1.get()));
        return pairs_step(o, nullptr, nullptr, 0, d_sk.get(), d_sz.get(), n, st, "pairs.tsv");
    }
    const auto distances = [&](float *d_out) {
        return kmc_sketch_distances(d_sk.get(), d_sz.get(), n, s, o.k, d_out, nullptr, nullptr, st);
    };
    const auto timers = [&](hipEvent_t t0, hipEvent_t t1) {
        printf("Sketch (s=%u): %.3f ms\n", s, ms_between(r0.get(), r1.get()));
        printf("Sketch distances: %.3f ms\n", ms_between(t0, t1));
    };
    std::vector<float> dist;
    if (int e = step2(o, n, st, true, dist, distances, timers)) return e;
    return write_csv(o.out_dir + "/sketch_results.csv", dist) ? 1 : 0;
}

// --canonical --sketch S --sketch-direct: the canonical counter never runs
int run_sketch_direct(const Options &o, const Records &r, hipStream_t st) {
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    return sketch_step(o, [&](uint32_t s, uint64_t *d_sk, uint32_t *d_sz) {
        return kmc_sketch_from_sequences(r.data.get(), r.idx.get(), r.n, r.bytes, o.k, flags, s,
                                         KMC_SKETCH_DEFAULT_SEED, d_sk, d_sz, nullptr, 0, st);
    }, r.n, st);
}

// the table of --min-abundance: --accum-slots, or the library's default for sketch size s
uint32_t accum_log2_slots(const Options &o, uint32_t s) {
    uint32_t lg = (uint32_t)o.accum_slots;
    if (lg == 0)
        for (lg = KMC_SKETCH_ACCUM_MIN_LOG2_SLOTS; (1ull << lg) < (uint64_t)KMC_SKETCH_ACCUM_DEFAULT_SLOTS_PER_VALUE * s;) ++lg;
    return lg;
}

// the accumulator's level for `bytes` added to a table of 2^lg slots, the library's rule (kmc.h):
// the smallest j with ceil(bytes / 2^j) <= 2^lg / 4; adds of no record do not count
uint32_t accum_level(uint64_t bytes, uint32_t lg) {
    uint32_t j = 0;
    while (((bytes + ((1ull << j) - 1)) >> j) > (1ull << (lg - 2))) ++j;
    return j;
}

// --per-file --min-abundance M: every file is one pass of the accumulator, reset in between;
// a FASTQ file batch by batch, every add on st behind its batch's parse (the next batch's
// writes are ordered behind that add), a FASTA file loaded whole and added in one call
// `inputs`: the files are the command's main inputs, whose spectra --spectrum writes.  With
// --min-abundance auto every file's spectrum is read back before its finish, whose M it gives.
int accum_files(const Options &o, const std::vector<std::string> &files, const char *what, bool inputs, uint32_t s,
                uint64_t *d_sk, uint32_t *d_sz, hipStream_t st) {
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    const uint32_t lg = accum_log2_slots(o, s);
    kmc_sketch_accum *acc = nullptr;
    KMCCHK(kmc_sketch_accum_create(s, o.k, flags, KMC_SKETCH_DEFAULT_SEED, lg, &acc));
    const Accum accum(acc);
    DevBuf<uint64_t> d_stats, d_hist, d_sstats;
    HIPCHK(dev_alloc(d_stats, 4));
    const bool written = inputs && o.spectrum > 0, taken = written || o.min_abundance_auto;
    const uint32_t B = o.spectrum > 0 ? (uint32_t)o.spectrum : 256u;
    std::vector<uint64_t> hist(B, 0);
    File f_hist, f_sum;
    if (taken) {
        HIPCHK(dev_alloc(d_hist, B));
        HIPCHK(dev_alloc(d_sstats, 4));
    }
    if (written) {
        f_hist.reset(fopen((o.out_dir + "/spectrum.tsv").c_str(), "w"));
        f_sum.reset(fopen((o.out_dir + "/spectrum_summary.tsv").c_str(), "w"));
        if (!f_hist || !f_sum) return fprintf(stderr, "kmc: cannot write %s/spectrum.tsv\n", o.out_dir.c_str()), 1;
    }
    for (size_t f = 0; f < files.size(); ++f) {
        const std::string &path = files[f];
        uint64_t records = 0, bytes = 0, batches = 0;
        KMCCHK(kmc_sketch_accum_reset(acc, st));
        FastqReader reader;  // (its buffers, or the loaded file's, live until the file's synchronisation)
        Records r;
        if (is_fastq(o, path)) {
            kmc_fastq_reader *rd = nullptr;
            const int orc = kmc_fastq_open(path.c_str(), o.batch, &rd);
            if (orc) return fprintf(stderr, "kmc: %s: %s\n", path.c_str(), kmc_error_string(orc)), 1;
            reader.reset(rd);
            for (;;) {
                const char *d_data = nullptr;
                const int64_t *d_idx = nullptr;
                uint64_t nb = 0, ns = 0;
                const int rc = kmc_fastq_next(rd, &d_data, &nb, &d_idx, &ns, st);
                if (rc == KMC_ERR_FORMAT) return malformed(path, ns);
                KMCCHK(rc);
                if (!d_data) break;
                KMCCHK(kmc_sketch_accum_add(acc, d_data, d_idx, ns, nb, st));
                records += ns;
                bytes += nb;
                ++batches;
            }
        } else {
            Options of = o;
            of.input = path;
            of.quiet = true;
            if (int e = load(of, st, r)) return e;
            KMCCHK(kmc_sketch_accum_add(acc, r.data.get(), r.idx.get(), r.n, r.bytes, st));
            records = r.n;
            bytes = r.bytes;
            batches = 1;
        }
        uint32_t M = (uint32_t)o.min_abundance;
        uint64_t sstats[4] = {0, 0, 0, 0};
        kmc_spectrum_summary sum;
        if (taken) {
            KMCCHK(kmc_spectrum_from_accum(acc, B, d_hist.get(), d_sstats.get(), st));
            HIPCHK(hipMemcpyAsync(hist.data(), d_hist.get(), (size_t)B * 8, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(sstats, d_sstats.get(), sizeof sstats, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            KMCCHK(kmc_spectrum_summarize(hist.data(), B, sstats[1], &sum));
            if (o.min_abundance_auto) M = sum.min_abundance;
        }
        KMCCHK(kmc_sketch_accum_finish(acc, M, d_sk + f * s, d_sz + f, d_stats.get(), st));
        uint32_t size = 0;
        uint64_t stats[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(&size, d_sz + f, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stats, d_stats.get(), sizeof stats, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // before the file's buffers go
        const uint32_t j = accum_level(bytes, lg);
        if (!o.quiet) {
            printf("%s %zu: %s: %" PRIu64 " records, %" PRIu64 " batches, sketch size %u, j %u, complete %d", what, f,
                   path.c_str(), records, batches, size, j, (int)stats[0]);
            if (o.min_abundance_auto) printf(", min-abundance %u", M);
            printf("\n");
        }
        if (written) {
            for (uint32_t c = 1; c < B; ++c)
                if (hist[c] > 0)
                    fprintf(f_hist.get(), "%zu\t%u\t%" PRIu64 "\t%.6g\n", f, c, hist[c], sum.scale * (double)hist[c]);
            fprintf(f_sum.get(),
                    "%zu\t%s\t%" PRIu64 "\t%.6g\t%" PRIu64 "\t%" PRIu64 "\t%.6g\t%.6g\t%u\t%u\t%u\t%u\t%.6g\n", f,
                    path.c_str(), sstats[1], sum.scale, sstats[2], sstats[3], sum.distinct, sum.total, sum.valley,
                    sum.peak, M, sum.saturated, sum.genome_size);
        }
        if (!stats[0])
            return fprintf(stderr,
                           "kmc: %s: the table of 2^%u slots kept only %u of %u sketch values with abundance >= %u "
                           "(%" PRIu64 " k-mers tracked below hash %" PRIu64 "): raise --accum-slots\n",
                           path.c_str(), lg, size, s, M, stats[2], stats[1]), 1;
    }
    if (written && ((fclose(f_hist.release()) != 0) | (fclose(f_sum.release()) != 0)))
        return fprintf(stderr, "kmc: cannot write %s/spectrum.tsv\n", o.out_dir.c_str()), 1;
    return 0;
}

// --per-file: every file is one group of all its records; file f's call writes row f
// (rows of separate calls concatenate), so one file at a time is resident
int sketch_files(const Options &o, const std::vector<std::string> &files, const char *what, bool inputs, uint32_t s,
                 uint64_t *d_sk, uint32_t *d_sz, hipStream_t st) {
    if (o.min_abundance > 0) return accum_files(o, files, what, inputs, s, d_sk, d_sz, st);
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    DevBuf<int64_t> d_grp;
    HIPCHK(dev_alloc(d_grp, 2));
    for (size_t f = 0; f < files.size(); ++f) {
        Options of = o;
        of.input = files[f];
        of.quiet = true;  // (the loader's lines are the single-file run's)
        Records r;
        if (int e = load(of, st, r)) return e;
        uint32_t size = 0;
        if (r.n == 0) {  // no record: the empty sketch
            HIPCHK(hipMemsetAsync(d_sk + f * s, 0xFF, (size_t)s * 8, st));
            HIPCHK(hipMemsetAsync(d_sz + f, 0, 4, st));
        } else {
            const int64_t grp[2] = {0, (int64_t)r.n};
            HIPCHK(hipMemcpyAsync(d_grp.get(), grp, sizeof grp, hipMemcpyHostToDevice, st));
            KMCCHK(kmc_sketch_from_sequences_grouped(r.data.get(), r.idx.get(), r.n, r.bytes, d_grp.get(), 1, o.k,
                                                     flags, s, KMC_SKETCH_DEFAULT_SEED, d_sk + f * s, d_sz + f,
                                                     nullptr, 0, st));
            HIPCHK(hipMemcpyAsync(&size, d_sz + f, 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));  // before the file's buffers go
        if (!o.quiet)
            printf("%s %zu: %s: %" PRIu64 " records, sketch size %u\n", what, f, files[f].c_str(), r.n, size);
    }
    return 0;
}

// f(data, idx, records, bytes) over the batches of one file on st: a FASTQ file batch by
// batch through the reader (the next batch's writes are ordered behind what f put on st), a
// FASTA file loaded whole, one batch.  The batch's buffers live until f returns.  With
// `reader` the FASTQ reader is opened with `flags` and *reader is it while f runs (null for FASTA).
template <class F>
int for_each_batch(const Options &o, const std::string &path, hipStream_t st, uint64_t *batches, F &&f,
                   unsigned flags = 0, kmc_fastq_reader **current = nullptr) {
    *batches = 0;
    if (current) *current = nullptr;
    if (is_fastq(o, path)) {
        kmc_fastq_reader *rd = nullptr;
        const int orc = kmc_fastq_open_ex(path.c_str(), o.batch, flags, &rd);
        if (orc) return fprintf(stderr, "kmc: %s: %s\n", path.c_str(), kmc_error_string(orc)), 1;
        const FastqReader reader(rd);
        if (current) *current = rd;
        for (;;) {
            const char *d_data = nullptr;
            const int64_t *d_idx = nullptr;
            uint64_t nb = 0, ns = 0;
            const int rc = kmc_fastq_next(rd, &d_data, &nb, &d_idx, &ns, st);
            if (rc == KMC_ERR_FORMAT) return malformed(path, ns);
            KMCCHK(rc);
            if (!d_data) break;
            if (int e = f(d_data, d_idx, ns, nb)) return e;
            ++*batches;
        }
        return 0;
    }
    Options of = o;
    of.input = path;
    of.quiet = true;
    Records r;
    if (int e = load(of, st, r)) return e;
    *batches = 1;
    return f(r.data.get(), r.idx.get(), r.n, r.bytes);
}

// --recruit: the input files are one k-mer set in the abundance accumulator; every record
// of every --recruit file is matched against it, batch by batch on st
int run_recruit(const Options &o, hipStream_t st) {
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    const uint32_t lg = (uint32_t)o.accum_slots, M = o.min_abundance > 0 ? (uint32_t)o.min_abundance : 1u;
    kmc_sketch_accum *acc = nullptr;
    KMCCHK(kmc_sketch_accum_create(1, o.k, flags, KMC_SKETCH_DEFAULT_SEED, lg, &acc));
    const Accum accum(acc);
    std::vector<std::string> files{o.input};
    files.insert(files.end(), o.more_inputs.begin(), o.more_inputs.end());
    uint64_t added = 0;  // the bytes of all adds: the level j is the library's rule for them (kmc.h)
    for (size_t f = 0; f < files.size(); ++f) {
        uint64_t records = 0, batches = 0;
        const int e = for_each_batch(o, files[f], st, &batches,
                                     [&](const char *d, const int64_t *idx, uint64_t ns, uint64_t nb) {
            KMCCHK(kmc_sketch_accum_add(acc, d, idx, ns, nb, st));
            HIPCHK(hipStreamSynchronize(st));  // before the batch's buffers go
            records += ns;
            if (ns > 0) added += nb;  // (the library leaves N as it is for a call of no record)
            return 0;
        });
        if (e) return e;
        if (!o.quiet)
            printf("Set %zu: %s: %" PRIu64 " records, %" PRIu64 " batches\n", f, files[f].c_str(), records, batches);
    }
    if (o.classify)  // every add is done: the inputs once more, file f is source f
        for (size_t f = 0; f < files.size(); ++f) {
            uint64_t batches = 0;
            KMCCHK(kmc_label_accum(acc, nullptr, nullptr, 0, 0, (uint32_t)f, st));  // (a file of no record)
            const int e = for_each_batch(o, files[f], st, &batches,
                                         [&](const char *d, const int64_t *idx, uint64_t ns, uint64_t nb) {
                KMCCHK(kmc_label_accum(acc, d, idx, ns, nb, (uint32_t)f, st));
                HIPCHK(hipStreamSynchronize(st));  // before the batch's buffers go
                return 0;
            });
            if (e) return e;
        }
    // the level only says whether `limit` is its bound or a refused k-mer's hash (the warning below);
    // limit and exact themselves are always the library's
    const uint32_t j = accum_level(added, lg);
    const uint64_t bound = j == 0 ? UINT64_MAX : 1ull << (64 - j);
    File f_rec(fopen((o.out_dir + "/read_matches.tsv").c_str(), "w"));
    File f_sum(fopen((o.out_dir + "/read_matches_summary.tsv").c_str(), "w"));
    if (!f_rec || !f_sum) return fprintf(stderr, "kmc: cannot write %s/read_matches.tsv\n", o.out_dir.c_str()), 1;
    fprintf(f_rec.get(), "file\trecord\twindows\tsampled\thits\n");
    fprintf(f_sum.get(), "file\tpath\trecords\tlisted\tlimit\texact\tsampled\thits\n");
    // --classify: the votes of one batch (best, best_hits, next_hits: three arrays of `cap`) and their files
    const uint32_t nsrc = o.classify ? (uint32_t)files.size() : 0u;
    File f_src, f_ssum;
    DevBuf<uint32_t> d_vote;
    std::vector<uint32_t> vote;
    if (o.classify) {
        f_src.reset(fopen((o.out_dir + "/read_sources.tsv").c_str(), "w"));
        f_ssum.reset(fopen((o.out_dir + "/read_sources_summary.tsv").c_str(), "w"));
        if (!f_src || !f_ssum) return fprintf(stderr, "kmc: cannot write %s/read_sources.tsv\n", o.out_dir.c_str()), 1;
        fprintf(f_src.get(), "file\trecord\twindows\tsampled\thits\tsource\tsource_hits\tnext_hits\n");
        fprintf(f_ssum.get(), "file\tsource\tpath\tbest\tassigned\n");
        HIPCHK(dev_alloc(d_vote, 3));
    }
    DevBuf<uint32_t> d_out;  // windows, sampled, hits of one batch: three arrays of `cap`
    DevBuf<uint64_t> d_stats;
    DevBuf<int64_t> d_none;  // the offsets of a call of no record
    HIPCHK(dev_alloc(d_stats, 4));
    HIPCHK(dev_alloc(d_out, 3));  // (never null: a batch or a file may hold no record)
    HIPCHK(dev_alloc(d_none, 1));
    HIPCHK(hipMemsetAsync(d_none.get(), 0, sizeof(int64_t), st));
    uint64_t cap = 1;
    std::vector<uint32_t> out;
    // what the set is, for a file of no batch: the stats of a match of no record
    uint64_t of_set[4] = {0, 0, 0, 0};
    KMCCHK(kmc_match_from_accum(acc, nullptr, d_none.get(), 0, 0, M, nullptr, nullptr, d_out.get(), d_stats.get(), st));
    HIPCHK(hipMemcpyAsync(of_set, d_stats.get(), sizeof of_set, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool lost = false;
    // --write-recruited, --write-rest: the flags and the kept bytes of one batch, and the way to the file
    const bool writing = o.write_recruited || o.write_rest || o.write_sources;
    DevBuf<uint32_t> d_keep;
    DevBuf<char> d_sel;
    DevBuf<uint64_t> d_counts;
    DevBuf<uint32_t> d_assign;  // --write-sources: the flags of one source
    uint64_t keep_cap = 0, sel_cap = 0, assign_cap = 0;
    kmc::Drainer drainer;
    if (writing) {
        HIPCHK(dev_alloc(d_counts, 2));
        KMCCHK(drainer.init((size_t)std::min<uint64_t>(o.batch ? o.batch : (256ull << 20), kmc::kStageChunk)));
    }
    for (size_t f = 0; f < o.recruit.size(); ++f) {
        uint64_t records = 0, listed = 0, batches = 0;
        uint64_t total[4] = {of_set[0], of_set[1], 0, 0};
        // [0]: recruited_<f>.fastq (invert 0), [1]: rest_<f>.fastq (invert 1)
        Fd fd[2];
        std::string name[2];
        uint64_t written[2] = {0, 0};
        for (int w = 0; w < 2; ++w) {
            if (!(w == 0 ? o.write_recruited : o.write_rest)) continue;
            name[w] = o.out_dir + (w == 0 ? "/recruited_" : "/rest_") + std::to_string(f) + ".fastq";
            fd[w].reset(open(name[w].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666));
            if (fd[w].get() < 0) return fprintf(stderr, "kmc: cannot write %s\n", name[w].c_str()), 1;
        }
        // --classify: per source the listed records with it as best and those of them assigned; [nsrc]: to none
        std::vector<uint64_t> n_best(nsrc + 1, 0), n_assigned(nsrc + 1, 0), src_written(nsrc, 0);
        std::vector<Fd> src_fd(o.write_sources ? nsrc : 0);
        std::vector<std::string> src_name(src_fd.size());
        for (size_t g = 0; g < src_fd.size(); ++g) {
            src_name[g] = o.out_dir + "/source_" + std::to_string(f) + "_" + std::to_string(g) + ".fastq";
            src_fd[g].reset(open(src_name[g].c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666));
            if (src_fd[g].get() < 0) return fprintf(stderr, "kmc: cannot write %s\n", src_name[g].c_str()), 1;
        }
        kmc_fastq_reader *rd = nullptr;
        const int e = for_each_batch(o, o.recruit[f], st, &batches,
                                     [&](const char *d, const int64_t *idx, uint64_t ns, uint64_t nb) {
            if (ns > cap) {
                HIPCHK(dev_alloc(d_out, 3 * ns));
                if (o.classify) HIPCHK(dev_alloc(d_vote, 3 * ns));
                cap = ns;
            }
            uint32_t *d_win = d_out.get(), *d_smp = d_win + cap, *d_hit = d_smp + cap;
            uint32_t *d_best = d_vote.get(), *d_bh = d_best + cap, *d_nh = d_bh + cap;  // (--classify only)
            if (o.classify) {
                KMCCHK(kmc_classify_from_accum(acc, d, idx, ns, nb, nsrc, M, d_win, d_smp, d_hit, d_best, d_bh, d_nh, nullptr,
                                               d_stats.get(), nullptr, 0, st));
                vote.resize(3 * ns);
                if (ns > 0) {
                    HIPCHK(hipMemcpyAsync(vote.data(), d_best, ns * 4, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpyAsync(vote.data() + ns, d_bh, ns * 4, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipMemcpyAsync(vote.data() + 2 * ns, d_nh, ns * 4, hipMemcpyDeviceToHost, st));
                }
            } else {
                KMCCHK(kmc_match_from_accum(acc, d, idx, ns, nb, M, d_win, d_smp, d_hit, d_stats.get(), st));
            }
            out.resize(3 * ns);
            uint64_t stats[4] = {0, 0, 0, 0};
            if (ns > 0) {
                HIPCHK(hipMemcpyAsync(out.data(), d_win, ns * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(out.data() + ns, d_smp, ns * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(out.data() + 2 * ns, d_hit, ns * 4, hipMemcpyDeviceToHost, st));
            }
            HIPCHK(hipMemcpyAsync(stats, d_stats.get(), sizeof stats, hipMemcpyDeviceToHost, st));
            if (writing) {  // the same rule on the device, then the selected raw text, once per output
                const char *d_raw = nullptr;
                const int64_t *d_ridx = nullptr;
                uint64_t raw_bytes = 0;
                KMCCHK(kmc_fastq_raw(rd, &d_raw, &raw_bytes, &d_ridx));
                if (ns > keep_cap) {
                    HIPCHK(dev_alloc(d_keep, ns));
                    keep_cap = ns;
                }
                if (raw_bytes > sel_cap) {
                    HIPCHK(dev_alloc(d_sel, raw_bytes));
                    sel_cap = raw_bytes;
                }
                KMCCHK(kmc_match_select(d_smp, d_hit, ns, (uint32_t)o.min_hits, o.min_fraction, d_keep.get(), nullptr, st));
                for (int w = 0; w < 2 && ns > 0; ++w) {
                    if (fd[w].get() < 0) continue;
                    uint64_t counts[2] = {0, 0};
                    KMCCHK(kmc_select_records(d_raw, d_ridx, ns, raw_bytes, d_keep.get(), w, d_sel.get(), sel_cap, nullptr,
                                              d_counts.get(), nullptr, 0, st));
                    HIPCHK(hipMemcpyAsync(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    const int wrc = drainer.drain(fd[w].get(), d_sel.get(), counts[1], st);
                    if (wrc == KMC_ERR_IO) return fprintf(stderr, "kmc: cannot write %s\n", name[w].c_str()), 1;
                    KMCCHK(wrc);
                    written[w] += counts[0];
                }
                // --write-sources: the listed records assigned to source g, through the same way
                for (size_t g = 0; g < src_fd.size() && ns > 0; ++g) {
                    uint64_t counts[2] = {0, 0};
                    if (ns > assign_cap) {
                        HIPCHK(dev_alloc(d_assign, ns));
                        assign_cap = ns;
                    }
                    KMCCHK(kmc_classify_select(d_keep.get(), d_best, d_bh, d_nh, ns, (uint32_t)g, (uint32_t)o.min_margin,
                                               d_assign.get(), nullptr, st));
                    KMCCHK(kmc_select_records(d_raw, d_ridx, ns, raw_bytes, d_assign.get(), 0, d_sel.get(), sel_cap, nullptr,
                                              d_counts.get(), nullptr, 0, st));
                    HIPCHK(hipMemcpyAsync(counts, d_counts.get(), sizeof counts, hipMemcpyDeviceToHost, st));
                    HIPCHK(hipStreamSynchronize(st));
                    const int wrc = drainer.drain(src_fd[g].get(), d_sel.get(), counts[1], st);
                    if (wrc == KMC_ERR_IO) return fprintf(stderr, "kmc: cannot write %s\n", src_name[g].c_str()), 1;
                    KMCCHK(wrc);
                    src_written[g] += counts[0];
                }
            }
            HIPCHK(hipStreamSynchronize(st));  // before the batch's buffers go
            total[0] = stats[0];
            total[1] = stats[1];
            total[2] += stats[2];
            total[3] += stats[3];
            for (uint64_t r = 0; r < ns; ++r) {
                const uint32_t win = out[r], smp = out[ns + r], hit = out[2 * ns + r];
                if (hit >= (uint64_t)o.min_hits && (double)hit >= o.min_fraction * (double)smp) {
                    fprintf(f_rec.get(), "%zu\t%" PRIu64 "\t%u\t%u\t%u\n", f, records + r, win, smp, hit);
                    ++listed;
                    if (o.classify) {  // kmc_classify_select's rule
                        const uint32_t best = vote[r], bh = vote[ns + r], nh = vote[2 * ns + r];
                        const bool none = best >= nsrc;  // KMC_CLASSIFY_NONE
                        fprintf(f_src.get(), "%zu\t%" PRIu64 "\t%u\t%u\t%u\t", f, records + r, win, smp, hit);
                        if (none) fprintf(f_src.get(), "-\t%u\t%u\n", bh, nh);
                        else fprintf(f_src.get(), "%u\t%u\t%u\n", best, bh, nh);
                        ++n_best[none ? nsrc : best];
                        ++n_assigned[!none && bh - nh >= (uint32_t)o.min_margin ? best : nsrc];
                    }
                }
            }
            records += ns;
            return 0;
        }, writing ? KMC_FASTQ_KEEP_RAW : 0u, &rd);
        if (e) return e;
        for (int w = 0; w < 2; ++w) {
            if (fd[w].get() < 0) continue;
            if (close(fd[w].release()) != 0) return fprintf(stderr, "kmc: cannot write %s\n", name[w].c_str()), 1;
            if (written[w] != (w == 0 ? listed : records - listed))  // the host's rule and the device's are one
                return fprintf(stderr, "kmc: %s holds %" PRIu64 " records, read_matches.tsv lists %" PRIu64 " of %" PRIu64 "\n",
                               name[w].c_str(), written[w], listed, records), 1;
        }
        fprintf(f_sum.get(), "%zu\t%s\t%" PRIu64 "\t%" PRIu64 "\t%" PRIu64 "\t%d\t%" PRIu64 "\t%" PRIu64 "\n", f,
                o.recruit[f].c_str(), records, listed, total[1], (int)total[0], total[2], total[3]);
        for (size_t g = 0; g < src_fd.size(); ++g) {
            if (close(src_fd[g].release()) != 0) return fprintf(stderr, "kmc: cannot write %s\n", src_name[g].c_str()), 1;
            if (src_written[g] != n_assigned[g])  // the host's rule and the device's are one
                return fprintf(stderr, "kmc: %s holds %" PRIu64 " records, read_sources.tsv assigns %" PRIu64 "\n",
                               src_name[g].c_str(), src_written[g], n_assigned[g]), 1;
        }
        if (o.classify) {
            for (uint32_t g = 0; g < nsrc; ++g)
                fprintf(f_ssum.get(), "%zu\t%u\t%s\t%" PRIu64 "\t%" PRIu64 "\n", f, g, files[g].c_str(), n_best[g],
                        n_assigned[g]);
            fprintf(f_ssum.get(), "%zu\t-\t-\t%" PRIu64 "\t%" PRIu64 "\n", f, n_best[nsrc], n_assigned[nsrc]);
        }
        if (!o.quiet)
            printf("Recruit %zu: %s: %" PRIu64 " records, %" PRIu64 " batches, %" PRIu64 " listed, j %u, exact %d\n", f,
                   o.recruit[f].c_str(), records, batches, listed, j, (int)total[0]);
        lost = lost || total[1] < bound;
    }
    if (lost)
        fprintf(stderr, "kmc: the table of 2^%u slots refused k-mers: the set is the sample below a smaller hash limit "
                        "than its level's (read_matches_summary.tsv); raise --accum-slots to keep more\n", lg);
    if ((fclose(f_rec.release()) != 0) | (fclose(f_sum.release()) != 0))
        return fprintf(stderr, "kmc: cannot write %s/read_matches.tsv\n", o.out_dir.c_str()), 1;
    if (o.classify && ((fclose(f_src.release()) != 0) | (fclose(f_ssum.release()) != 0)))
        return fprintf(stderr, "kmc: cannot write %s/read_sources.tsv\n", o.out_dir.c_str()), 1;
    return 0;
}

int run_per_file(const Options &o, hipStream_t st) {
    std::vector<std::string> files{o.input};
    files.insert(files.end(), o.more_inputs.begin(), o.more_inputs.end());
    return sketch_step(o, [&](uint32_t s, uint64_t *d_sk, uint32_t *d_sz) {
        return sketch_files(o, files, "File", true, s, d_sk, d_sz, st);
    }, files.size(), st);
}

// The sketch rows of a query or reference set: one per record of the one file, or
// (--per-file) one per file.
struct Rows {
    DevBuf<uint64_t> sk;
    DevBuf<uint32_t> sz;
    uint64_t n = 0;
};

int make_rows(const Options &o, const std::vector<std::string> &files, const char *what, bool announce, hipStream_t st,
              Rows &rows) {
    const uint32_t s = (uint32_t)o.sketch;
    if (o.per_file) {
        rows.n = files.size();
        HIPCHK(dev_alloc(rows.sk, rows.n * s));
        HIPCHK(dev_alloc(rows.sz, rows.n));
        // (announce: the command's inputs; the references of --screen get no spectrum)
        return sketch_files(o, files, what, announce && o.screen.empty(), s, rows.sk.get(), rows.sz.get(), st);
    }
    Options of = o;
    of.input = files[0];
    of.quiet = o.quiet || !announce;
    Records r;
    if (int e = load(of, st, r)) return e;
    rows.n = r.n;
    HIPCHK(dev_alloc(rows.sk, rows.n * s));
    HIPCHK(dev_alloc(rows.sz, rows.n));
    KMCCHK(kmc_sketch_from_sequences(r.data.get(), r.idx.get(), r.n, r.bytes, o.k, o.softmask ? KMC_CANON_SOFTMASK : 0u,
                                     s, KMC_SKETCH_DEFAULT_SEED, rows.sk.get(), rows.sz.get(), nullptr, 0, st));
    HIPCHK(hipStreamSynchronize(st));  // before the records go
    if (!o.quiet && !announce) printf("%s: %s: %" PRIu64 " records\n", what, files[0].c_str(), r.n);
    return 0;
}

// --query FILE: the inputs are the references; FILE's sketches are searched in them
int run_query(const Options &o, hipStream_t st) {
    std::vector<std::string> files{o.input};
    files.insert(files.end(), o.more_inputs.begin(), o.more_inputs.end());
    const uint32_t s = (uint32_t)o.sketch, top = (uint32_t)o.top;
    Rows R, Q;
    if (int e = make_rows(o, files, "Reference", true, st, R)) return e;
    if (int e = make_rows(o, {o.query}, "Query", false, st, Q)) return e;
    const uint64_t m = Q.n, n = R.n;
    if (o.pairs_set)  // Mash's dist -d of a query file against a collection
        return pairs_step(o, Q.sk.get(), Q.sz.get(), m, R.sk.get(), R.sz.get(), n, st, "query_pairs.tsv");
    Event t0 = make_event(), t1 = make_event();
    if (top == 0) {  // the whole rectangle
        DevBuf<float> d_out;
        HIPCHK(dev_alloc(d_out, m * n));
        HIPCHK(hipEventRecord(t0.get(), st));
        KMCCHK(kmc_sketch_distances_rect(Q.sk.get(), Q.sz.get(), m, R.sk.get(), R.sz.get(), n, s, o.k, d_out.get(),
                                         nullptr, nullptr, st));
        HIPCHK(hipEventRecord(t1.get(), st));
        HIPCHK(hipEventSynchronize(t1.get()));
        if (!o.quiet)
            printf("Query distances (%" PRIu64 " x %" PRIu64 "): %.3f ms\n", m, n, ms_between(t0.get(), t1.get()));
        std::vector<float> dist(m * n);
        if (m * n > 0) HIPCHK(hipMemcpy(dist.data(), d_out.get(), m * n * sizeof(float), hipMemcpyDeviceToHost));
        return write_csv(o.out_dir + "/query_distances.csv", dist) ? 1 : 0;
    }
    DevBuf<uint32_t> d_ref, d_sh, d_dn, d_cnt;
    DevBuf<float> d_dist;
    HIPCHK(dev_alloc(d_ref, m * top));
    HIPCHK(dev_alloc(d_sh, m * top));
    HIPCHK(dev_alloc(d_dn, m * top));
    HIPCHK(dev_alloc(d_dist, m * top));
    HIPCHK(dev_alloc(d_cnt, m));
    HIPCHK(hipEventRecord(t0.get(), st));
    KMCCHK(kmc_sketch_nearest(Q.sk.get(), Q.sz.get(), m, R.sk.get(), R.sz.get(), n, s, o.k, top,
                              (uint32_t)o.min_shared, d_ref.get(), d_sh.get(), d_dn.get(), d_dist.get(), d_cnt.get(),
                              nullptr, 0, st));
    HIPCHK(hipEventRecord(t1.get(), st));
    HIPCHK(hipEventSynchronize(t1.get()));
    if (!o.quiet)
        printf("Query search (%" PRIu64 " in %" PRIu64 ", top %u): %.3f ms\n", m, n, top,
               ms_between(t0.get(), t1.get()));
    std::vector<uint32_t> ref(m * top), sh(m * top), dn(m * top), cnt(m);
    std::vector<float> dist(m * top);
    if (m > 0) {
        HIPCHK(hipMemcpy(ref.data(), d_ref.get(), ref.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sh.data(), d_sh.get(), sh.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dn.data(), d_dn.get(), dn.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(dist.data(), d_dist.get(), dist.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnt.data(), d_cnt.get(), cnt.size() * 4, hipMemcpyDeviceToHost));
    }
    const std::string path = o.out_dir + "/query_results.tsv";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    for (uint64_t q = 0; q < m; ++q)
        for (uint32_t i = 0; i < cnt[q] && i < top; ++i) {
            const uint64_t at = q * top + i;
            fprintf(f, "%" PRIu64 "\t%u\t%u\t%u\t%u\t%f\n", q, i + 1, ref[at], sh[at], dn[at], dist[at]);
        }
    return fclose(f) == 0 ? 0 : 1;
}

// --screen FILE ...: the inputs are the references; every FILE's k-mers are counted into one
// index of the references' sketch values, one file resident at a time
int run_screen(const Options &o, hipStream_t st) {
    std::vector<std::string> files{o.input};
    files.insert(files.end(), o.more_inputs.begin(), o.more_inputs.end());
    const uint32_t s = (uint32_t)o.sketch;
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    Rows R;
    if (int e = make_rows(o, files, "Reference", true, st, R)) return e;
    const uint64_t n = R.n;
    const size_t index_bytes = kmc_sketch_screen_index_size(n, s);
    if (index_bytes == 0) return fprintf(stderr, "kmc: too many reference sketch values for one screen index\n"), 1;
    DevBuf<char> d_index;
    DevBuf<uint32_t> d_sh, d_med, d_all;
    DevBuf<float> d_id;
    Event b0 = make_event(), b1 = make_event(), c0 = make_event(), c1 = make_event(), r1 = make_event();
    const bool wta = o.winner_takes_all;
    if (wta) HIPCHK(dev_alloc(d_all, n));
    HIPCHK(dev_alloc(d_index, index_bytes));
    HIPCHK(dev_alloc(d_sh, n));
    HIPCHK(dev_alloc(d_med, n));
    HIPCHK(dev_alloc(d_id, n));
    HIPCHK(hipEventRecord(b0.get(), st));
    KMCCHK(kmc_sketch_screen_build(R.sk.get(), R.sz.get(), n, s, d_index.get(), index_bytes, st));
    HIPCHK(hipEventRecord(b1.get(), st));
    HIPCHK(hipEventSynchronize(b1.get()));
    if (!o.quiet)
        printf("Screen index (%" PRIu64 " references, s=%u, %zu bytes): %.3f ms\n", n, s, index_bytes,
               ms_between(b0.get(), b1.get()));
    for (const std::string &path : o.screen) {
        if (is_fastq(o, path)) {
            // streamed: every batch is counted on st behind its parse, and the next batch's writes
            // are ordered behind that count, so the host reads ahead while the GPU counts
            kmc_fastq_reader *rd = nullptr;
            const int orc = kmc_fastq_open(path.c_str(), o.screen_batch, &rd);
            if (orc) return fprintf(stderr, "kmc: %s: %s\n", path.c_str(), kmc_error_string(orc)), 1;
            const FastqReader reader(rd);
            uint64_t records = 0, bytes = 0, batches = 0;
            const auto w0 = std::chrono::steady_clock::now();
            for (;;) {
                const char *d_data = nullptr;
                const int64_t *d_idx = nullptr;
                uint64_t nb = 0, ns = 0;
                const int rc = kmc_fastq_next(rd, &d_data, &nb, &d_idx, &ns, st);
                if (rc == KMC_ERR_FORMAT) return malformed(path, ns);
                KMCCHK(rc);
                if (!d_data) break;
                KMCCHK(kmc_sketch_screen_count(d_index.get(), index_bytes, d_data, d_idx, ns, nb, o.k, flags,
                                               KMC_SKETCH_DEFAULT_SEED, st));
                records += ns;
                bytes += nb;
                ++batches;
            }
            HIPCHK(hipStreamSynchronize(st));  // before the reader's buffers go
            if (!o.quiet)
                printf("Screen: %s: %" PRIu64 " records, %" PRIu64 " bytes, %" PRIu64 " batches: %.3f ms\n", path.c_str(),
                       records, bytes, batches,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count());
            continue;
        }
        Options of = o;
        of.input = path;
        of.max_seqs = 0;
        of.host_loader = false;
        of.quiet = true;
        Records r;
        if (int e = load(of, st, r)) return e;
        HIPCHK(hipEventRecord(c0.get(), st));
        KMCCHK(kmc_sketch_screen_count(d_index.get(), index_bytes, r.data.get(), r.idx.get(), r.n, r.bytes, o.k, flags,
                                       KMC_SKETCH_DEFAULT_SEED, st));
        HIPCHK(hipEventRecord(c1.get(), st));
        HIPCHK(hipStreamSynchronize(st));  // before the file's buffers go
        if (!o.quiet)
            printf("Screen: %s: %" PRIu64 " records, %" PRIu64 " bytes: %.3f ms\n", path.c_str(), r.n, r.bytes,
                   ms_between(c0.get(), c1.get()));
    }
    HIPCHK(hipEventRecord(c1.get(), st));
    if (wta)  // (the library's own workspace)
        KMCCHK(kmc_sketch_screen_winners(d_index.get(), index_bytes, R.sk.get(), R.sz.get(), n, s, o.k, d_sh.get(),
                                         d_med.get(), d_id.get(), d_all.get(), nullptr, 0, st));
    else
        KMCCHK(kmc_sketch_screen_results(d_index.get(), index_bytes, R.sk.get(), R.sz.get(), n, s, o.k, d_sh.get(),
                                         d_med.get(), d_id.get(), st));
    HIPCHK(hipEventRecord(r1.get(), st));
    HIPCHK(hipEventSynchronize(r1.get()));
    if (!o.quiet) printf(wta ? "Screen winners: %.3f ms\n" : "Screen results: %.3f ms\n", ms_between(c1.get(), r1.get()));
    std::vector<uint32_t> sh(n), med(n), sz(n), all(wta ? n : 0);
    std::vector<float> ident(n);
    if (n > 0) {
        HIPCHK(hipMemcpy(sh.data(), d_sh.get(), n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(med.data(), d_med.get(), n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(sz.data(), R.sz.get(), n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(ident.data(), d_id.get(), n * 4, hipMemcpyDeviceToHost));
        if (wta) HIPCHK(hipMemcpy(all.data(), d_all.get(), n * 4, hipMemcpyDeviceToHost));
    }
    const std::string path = o.out_dir + "/screen_results.tsv";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path.c_str()), 1;
    for (uint64_t r = 0; r < n; ++r) {
        fprintf(f, "%" PRIu64 "\t%u\t%u\t%u\t%f", r, sh[r], std::min(sz[r], s), med[r], ident[r]);
        if (wta) fprintf(f, "\t%u", all[r]);
        if (o.per_file) fprintf(f, "\t%s", files[r].c_str());
        fputc('\n', f);
    }
    return fclose(f) == 0 ? 0 : 1;
}

// --canonical: the sparse counts, then their dump, step 2 on them and their sketches
int run_canonical(const Options &o, const Records &r, hipStream_t st) {
    const int k = o.k;
    const uint64_t n = r.n, cap = r.bytes > 0 ? r.bytes : 1;
    const unsigned flags = o.softmask ? KMC_CANON_SOFTMASK : 0u;
    DevBuf<uint64_t> d_keys, d_off;
    DevBuf<uint32_t> d_cnt;
    Event c0 = make_event(), c1 = make_event();
    HIPCHK(dev_alloc(d_keys, cap));
    HIPCHK(dev_alloc(d_cnt, cap));
    HIPCHK(dev_alloc(d_off, n + 1));
    uint64_t distinct = 0;
    HIPCHK(hipEventRecord(c0.get(), st));
    KMCCHK(kmc_count_canonical_hash(r.data.get(), r.idx.get(), n, k, flags, d_keys.get(), d_cnt.get(), cap,
                                    d_off.get(), &distinct, st));
    HIPCHK(hipEventRecord(c1.get(), st));
    HIPCHK(hipStreamSynchronize(st));
    if (!o.quiet) {
        printf("Canonical k=%d: %" PRIu64 " distinct (record, k-mer) pairs, %.3f ms\n", k, distinct,
               ms_between(c0.get(), c1.get()));
    }
    if (!o.counts_path.empty()) {
        std::vector<uint64_t> keys(distinct), off(n + 1);
        std::vector<uint32_t> cnt(distinct);
        if (distinct) {
            HIPCHK(hipMemcpy(keys.data(), d_keys.get(), distinct * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(cnt.data(), d_cnt.get(), distinct * 4, hipMemcpyDeviceToHost));
        }
        HIPCHK(hipMemcpy(off.data(), d_off.get(), (n + 1) * 8, hipMemcpyDeviceToHost));
        FILE *f = fopen(o.counts_path.c_str(), "w");
        if (!f) return fprintf(stderr, "kmc: cannot write %s\n", o.counts_path.c_str()), 1;
        for (uint64_t s = 0; s < n; ++s)
            for (uint64_t i = off[s]; i < off[s + 1]; ++i)
                fprintf(f, "%" PRIu64 "\t%s\t%u\n", s, canon_kmer(keys[i], k).c_str(), cnt[i]);
        if (fclose(f) != 0) return 1;
    }
    if (o.canon_distances) {
        // step 2 on the sparse lists: both CSVs hold the one vector (exact integer sums)
        const auto sparse = [&](float *d_mins) {
            return kmc_pair_distances_sparse(d_keys.get(), d_cnt.get(), d_off.get(), distinct, r.idx.get(), n, k,
                                             d_mins, nullptr, 0, st);
        };
        const auto timer = [](hipEvent_t t0, hipEvent_t t1) {
            const float t2 = ms_between(t0, t1);
            printf("Elapsed parallel step 2 timer: %g ms, %g secs\n", t2, t2 / 1000);
        };
        std::vector<float> mins;
        if (int e = step2(o, n, st, false, mins, sparse, timer)) return e;
        if (write_csv(o.out_dir + "/parallel_results.csv", mins)) return 1;
        if (write_csv(o.out_dir + "/sequential_results.csv", mins)) return 1;
    }
    if (o.sketch == 0) return 0;
    // sketches of the canonical lists and their Mash distances
    return sketch_step(o, [&](uint32_t s, uint64_t *d_sk, uint32_t *d_sz) {
        return kmc_sketch_from_counts(d_keys.get(), d_cnt.get(), d_off.get(), distinct, n, s, KMC_SKETCH_DEFAULT_SEED,
                                      (uint32_t)o.min_count, d_sk, d_sz, nullptr, 0, st);
    }, n, st);
}

// the dense histogram (k <= 13) and step 2 on it: the reference's flow
int run_dense(const Options &o, const Records &r, hipStream_t st) {
    const int k = o.k;
    const uint64_t n = r.n, nb = 1ull << (2 * k);
    DevBuf<int32_t> d_sum;
    DevBuf<int> d_idx32;
    Event s0 = make_event(), s1 = make_event();
    HIPCHK(dev_alloc(d_sum, nb * n));
    if (o.dropin) {
        if (r.bytes > (uint64_t)INT32_MAX) return fprintf(stderr, "kmc: --dropin needs < 2 GiB of sequence\n"), 1;
        std::vector<int> i32(r.hidx.begin(), r.hidx.end());
        HIPCHK(dev_alloc(d_idx32, n + 1));
        HIPCHK(hipMemcpy(d_idx32.get(), i32.data(), (n + 1) * sizeof(int), hipMemcpyHostToDevice));
    }

    // step 1 (main.cu:287-300)
    HIPCHK(hipEventRecord(s0.get(), st));
    std::vector<int32_t> hsum;
    if (o.dropin) {
        KMCCHK(sumKmereCoincidencesGlobalMemory_hip(r.data.get(), d_idx32.get(), (unsigned)n, d_sum.get(), st));
    } else if (o.gpus > 1) {
        // host-buffer multi-GPU count (shards + RCCL all-reduce), result on the host
        hsum.assign(nb * n, 0);
        KMCCHK(kmc_count_multi(kmc_fasta_data(r.fa.get()), r.hidx.data(), n, r.bytes, k, o.gpus, nullptr, hsum.data(),
                               nullptr));
        if (!hsum.empty())
            HIPCHK(hipMemcpyAsync(d_sum.get(), hsum.data(), hsum.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    } else {
        KMCCHK(kmc_count_dense(r.data.get(), r.idx.get(), n, r.bytes, k, d_sum.get(), nullptr, nullptr, 0, st));
    }
    HIPCHK(hipEventRecord(s1.get(), st));
    HIPCHK(hipEventSynchronize(s1.get()));
    if (o.gpus <= 1) {  // the deferred status of the (asynchronous) count on this device
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        KMCCHK(kmc_dense_status(dev));
    }
    const float ms1 = ms_between(s0.get(), s1.get());
    if (!o.quiet) {
        printf("Elapsed parallel timer step 1: %g ms, %g secs\n", ms1, ms1 / 1000);  // main.cu:300
    }

    if (o.distances) {
        // step 2 (main.cu:326-344).  The reference writes both files for diffing (main.cu:178,
        // 194-202, 216, 351-358): sequential_results.csv holds the CPU path's exact integer sums
        // (`exact`), parallel_results.csv the GPU path's (the same, or `reference`'s float sums)
        const auto exact = [&](float *d_mins) {
            return kmc_pair_distances(d_sum.get(), n, r.idx.get(), n, k, d_mins, nullptr, 0, st);
        };
        const auto reference = [&](float *d_mins) {  // --dropin: one launch per record
            int e = hipMemsetAsync(d_mins, 0, n * (n - 1) / 2 * sizeof(float), st);
            for (uint64_t i = 0; i < n && !e; ++i) {
                e = minKmeres2_hip(d_sum.get(), d_mins, (int)n, (int)i, d_idx32.get(), st);
                if (!e) e = hipStreamSynchronize(st);  // main.cu:328
            }
            return e;
        };
        const auto timers = [&](hipEvent_t t0, hipEvent_t t1) {
            const float t2 = ms_between(t0, t1), tt = ms_between(s0.get(), t1);
            printf("Elapsed parallel step 2 timer: %g ms, %g secs\n", t2, t2 / 1000);  // main.cu:344
            printf("Total time elapsed parallel: %g ms, %g secs\n", tt, tt / 1000);    // main.cu:350
        };
        std::vector<float> mins, seq;
        const int e2 = o.dropin ? step2(o, n, st, false, mins, reference, timers)
                                : step2(o, n, st, false, mins, exact, timers);
        if (e2) return e2;
        if (o.dropin)  // untimed
            if (int e = step2(o, n, st, false, seq, exact, [](hipEvent_t, hipEvent_t) {})) return e;
        if (write_csv(o.out_dir + "/parallel_results.csv", mins)) return 1;
        if (write_csv(o.out_dir + "/sequential_results.csv", o.dropin ? seq : mins)) return 1;
    }
    if (!o.counts_path.empty()) {
        if (hsum.empty() && nb * n > 0) {
            hsum.resize(nb * n);
            HIPCHK(hipMemcpy(hsum.data(), d_sum.get(), hsum.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        if (write_counts(o.counts_path, hsum, n, k)) return 1;
    }
    return 0;
}

int run(const Options &o) {
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fprintf(stderr, "kmc: no HIP device\n"), 1;
    if (o.gpus > ndev) return fprintf(stderr, "kmc: --gpus %d but %d device(s)\n", o.gpus, ndev), 1;
    HIPCHK(hipSetDevice(0));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreate(&s));
    const Stream st(s);
    if (!o.query.empty()) return run_query(o, s);
    if (!o.screen.empty()) return run_screen(o, s);
    if (!o.recruit.empty()) return run_recruit(o, s);
    if (o.per_file) return run_per_file(o, s);
    Records r;  // (after the stream: released before it)
    if (int e = load(o, s, r)) return e;
    if (!o.canonical) return run_dense(o, r, s);
    return o.sketch_direct ? run_sketch_direct(o, r, s) : run_canonical(o, r, s);
}

// `kmc synth OUT.fa RECORDS LENGTH [SEED]`: the SURVEY.md §8(d) benchmark input as a
// FASTA file: records of LENGTH bases in 80 columns, '>r%04d' headers, records
// separated by one blank line (the importSeqs dialect, also read by NoNL), no
// final blank line.  Base g of the concatenated records is "ACGT"[(x_{g/32} >>
// 2(g%32)) & 3], x_n = splitmix64 output n (kmc_synth_fill's stream, so the parsed
// buffer equals kmc_synth_fill's).  Lines are generated by host threads.
int synth_main(int argc, char **argv) {
    if (argc < 5) return fprintf(stderr, "usage: kmc synth OUT.fa RECORDS LENGTH [SEED]\n"), 2;
    const char *path = argv[2];
    const uint64_t nrec = strtoull(argv[3], nullptr, 10), len = strtoull(argv[4], nullptr, 10);
    const uint64_t seed = argc > 5 ? strtoull(argv[5], nullptr, 0) : 0x5EED0008ull;
    FILE *f = fopen(path, "wb");
    if (!f) return fprintf(stderr, "kmc: cannot write %s\n", path), 1;
    const unsigned nth = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    constexpr uint64_t kBlockBases = 80ull << 20;  // whole lines per block
    std::vector<std::string> buf(nth);
    for (uint64_t r = 0; r < nrec; ++r) {
        char hdr[32];
        snprintf(hdr, sizeof hdr, "%s>r%04llu\n", r ? "\n" : "", (unsigned long long)r);
        fputs(hdr, f);
        for (uint64_t b0 = 0; b0 < len; b0 += kBlockBases * nth) {
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nth; ++t) {
                th.emplace_back([&, t]() {
                    std::string &o = buf[t];
                    o.clear();
                    const uint64_t lo = b0 + t * kBlockBases;
                    if (lo >= len) return;
                    const uint64_t hi = std::min(len, lo + kBlockBases);
                    o.reserve((hi - lo) + (hi - lo) / 80 + 2);
                    for (uint64_t i = lo; i < hi; i += 80) {
                        const uint64_t e = std::min(hi, i + 80);
                        uint64_t xn = ~0ull, x = 0;
                        for (uint64_t j = i; j < e; ++j) {
                            const uint64_t g = r * len + j;
                            if ((g >> 5) != xn) x = kmc::splitmix64_at(seed, xn = g >> 5);
                            o.push_back("ACGT"[(x >> (2 * (g & 31))) & 3]);
                        }
                        o.push_back('\n');
                    }
                });
            }
            for (auto &x : th) x.join();
            for (unsigned t = 0; t < nth; ++t)
                if (!buf[t].empty() && fwrite(buf[t].data(), 1, buf[t].size(), f) != buf[t].size())
                    return fclose(f), fprintf(stderr, "kmc: write failed\n"), 1;
        }
    }
    return fclose(f) == 0 ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && std::string(argv[1]) == "synth") return synth_main(argc, argv);
    Options o;
    const int rc = parse(argc, argv, o);
    if (rc) return rc;
    return run(o);
}
