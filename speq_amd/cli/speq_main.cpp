// `speq` command line: index | scan | all. Host C++ (reference layers L5/L4/L3) calling the
// MI355X scan path only through the C ABI of libspeq_scan.so (include/speq_scan.h).
//
//   main                        /root/reference/src/main.cpp:15-40
//   speq::fm::index             /root/reference/src/fm_indexer.cpp:55-111
//   speq::scan::async_one/two   /root/reference/src/fm_scanner.cpp:5-32 and the four mode variants
//   .dat cache                  /root/reference/src/fm_scanner.cpp:79-135, :1561-1571
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

#include "args.hpp"
#include "host_io.hpp"
#include "speq_scan.h"

namespace fs = std::filesystem;

namespace speq::args {

namespace {
const char* HELP =
    "speq - Species PErcent Quantifier (MI355X build)\n"
    "usage: speq [index|scan|all] [options]\n"
    "  -1, --forward FILE        FASTQ of (forward) reads\n"
    "  -2, --reverse FILE        FASTQ of reverse mates (paired mode)\n"
    "  -r, --reference FILE      reference sequences (FASTA)\n"
    "  -g, --groups FILE         groupings of reference sequences\n"
    "  -x, --index FILE          index file (default output.idx)\n"
    "  -o, --output FILE         output file of percentages (default output.txt)\n"
    "  -f, --force               overwrite existing output files\n"
    "  -k, --kmer N              k-mer size (default 70)\n"
    "  -t, --threads N           host threads (default 2)\n"
    "      --precision-cutoff X  EM convergence threshold (default 1e-6)\n"
    "      --phred-cutoff N      a window passes iff min(Q) > N (default 30)\n"
    "      --fixed-accuracy X    fixed per-base accuracy in [0,1]; 0 = Phred-weighted (default)\n"
    "      --prefix-q N          q-mer lookup tables of the FM-index, lengths N, N-1, N-2 (default 12, 0 = off)\n"
    "      --pair-steps 0|1      two-base LF planes in the FM-index (default 1)\n"
    "      --label-table auto|0|1 per-position group/run table: one-load classification (default auto:\n"
    "                            when the collection has >= 4 M symbols)\n"
    "      --gpu-build auto|0|1  build the suffix array on the GPU (default auto: when one is visible)\n"
    "      --triple-steps auto|0|1 three-base LF planes in the FM-index (10.7 B per symbol; default auto:\n"
    "                            on below ~400 M symbols)\n"
    "      --device N            GPU ordinal (default $LOCAL_RANK or 0)\n"
    "      --gpus N              scan: shard the reads over GPUs 0..N-1 (default 1; 0 = every visible GPU)\n"
    "      --devices I,J,...     scan: shard the reads over these GPU ordinals (repeats allowed)\n"
    "      --group-sets FILE     scan: after the scan, one more pass over the reads writes FILE: one line per distinct\n"
    "                            set of groups that a read's (pair's) unique k-mers name, as units, number of groups,\n"
    "                            names ('-' = none); the lines of 2 or more groups are the fusion map\n"
    "      --marker-coverage FILE scan: after the scan, one more pass over the reads writes FILE: per group, how many of\n"
    "                            its unique k-mers (markers) the reads cover and how deep: name, markers, observed,\n"
    "                            breadth, hits, mean_depth, expected_breadth, max_depth, d0..d7 (tab-separated); a\n"
    "                            breadth far below expected_breadth means copies of few k-mers, not the variant\n"
    "      --marker-track FILE   scan: after the scan, one more pass over the reads (the same one as --marker-coverage's\n"
    "                            when both are given) writes FILE: per reference record and bin of --track-bin window\n"
    "                            starts, where the covered markers lie: record (0-based, FASTA order), group, start,\n"
    "                            end, markers, observed, breadth, hits, mean_depth, max_depth (tab-separated); both\n"
    "                            strands of a k-mer count at its place in the record\n"
    "      --track-bin N         window starts per bin of --marker-track, 1..1048576 (default 100)\n"
    "      --bootstrap FILE      scan: after the scan, one more pass over the reads resamples them (Poisson bootstrap\n"
    "                            of the reads, or pairs) and writes FILE: name, percent, mean, se, lo, hi, used\n"
    "                            (tab-separated): the interval of each group's initial percentage, the first vector\n"
    "                            the run prints, from unique k-mers; the EM-refined percentages are not covered\n"
    "      --bootstrap-em FILE   scan: the same pass also fills one EM histogram per resampling and refines each with\n"
    "                            the run's --precision-cutoff and --max-em-iterations; FILE has the same columns for\n"
    "                            the EM-refined percentages, the vector written to -o\n"
    "      --bootstrap-replicates N  resamplings, 1..1024 (default 200)\n"
    "      --bootstrap-seed S    seed of the resampling weights (default 1)\n"
    "      --bootstrap-level L   two-sided level of lo..hi, in (0,1) (default 0.95)\n"
    "      --dedup FILE          scan: after the scan, two more passes over the reads count every distinct read (pair)\n"
    "                            once: reads (pairs) of the same bases, whatever their qualities, are duplicates and the\n"
    "                            first one in the file is kept. FILE: '#' lines with units, distinct, duplicates,\n"
    "                            duplicate_fraction, max_multiplicity and multiplicity_hist, then name, percent,\n"
    "                            percent_dedup, refined, refined_dedup (tab-separated): the run's initial and EM-refined\n"
    "                            percentages beside the same from the deduplicated reads\n"
    "one process per GPU: run under a launcher that sets WORLD_SIZE > 1, RANK and LOCAL_RANK (e.g. torchrun\n"
    "--no-python bin/speq scan ...): each rank scans its share of the reads on GPU $LOCAL_RANK and the counts are\n"
    "summed with RCCL; rank 0 prints and writes the results ($SPEQ_RENDEZVOUS: the id file, default under /tmp)\n";

template <typename T>
T to_number(const std::string& opt, const std::string& v) {
    try {
        size_t used = 0;
        if constexpr (std::is_same_v<T, double>) {
            double x = std::stod(v, &used);
            if (used != v.size()) throw std::invalid_argument("");
            return x;
        } else if constexpr (std::is_same_v<T, int>) {
            long x = std::stol(v, &used);
            if (used != v.size()) throw std::invalid_argument("");
            return (int)x;
        } else {
            if (!v.empty() && v[0] == '-') throw std::invalid_argument("");
            unsigned long x = std::stoul(v, &used);
            if (used != v.size()) throw std::invalid_argument("");
            return (T)x;
        }
    } catch (const std::exception&) {
        throw ParseError("Value parse failed for " + opt + ": " + v);
    }
}
}  // namespace

CmdArguments parse(int argc, char** argv) {
    CmdArguments a;
    if (argc < 2) throw ParseError("missing sub-command (index, scan or all)");
    const std::string sub = argv[1];
    if (sub == "-h" || sub == "--help") {
        std::cout << HELP;
        return a;
    }
    if (sub == "index") a.is_indexer = true;
    else if (sub == "scan") a.is_scanner = true;
    else if (sub == "all") a.is_indexer = a.is_scanner = true;
    else throw ParseError("You specified an unknown subcommand! Available subcommands are: [index, scan, all]");
    const bool allow_reads = a.is_scanner, allow_refs = a.is_indexer;
    for (int i = 2; i < argc; ++i) {
        std::string opt = argv[i], val;
        const size_t eq = opt.find('=');
        bool has_inline = opt.rfind("--", 0) == 0 && eq != std::string::npos;
        if (has_inline) {
            val = opt.substr(eq + 1);
            opt = opt.substr(0, eq);
        }
        auto value = [&]() -> std::string {
            if (has_inline) return val;
            if (i + 1 >= argc) throw ParseError("Missing value for option " + opt);
            return argv[++i];
        };
        if (opt == "-h" || opt == "--help") { std::cout << HELP; a.is_parsed = false; return a; }
        else if (opt == "-f" || opt == "--force") a.is_force = true;
        else if (allow_reads && (opt == "-1" || opt == "--forward")) a.in_file_reads_path_1 = value();
        else if (allow_reads && (opt == "-2" || opt == "--reverse")) a.in_file_reads_path_2 = value();
        else if (allow_refs && (opt == "-r" || opt == "--reference")) a.in_file_references = value();
        else if (allow_refs && (opt == "-g" || opt == "--groups")) a.in_file_references_groups = value();
        else if (opt == "-x" || opt == "--index") a.io_file_index = value();
        else if (opt == "-o" || opt == "--output") a.out_file_path = value();
        else if (allow_reads && (opt == "-k" || opt == "--kmer")) a.kmer = to_number<unsigned>(opt, value());
        else if (opt == "-t" || opt == "--threads") a.threads = to_number<unsigned>(opt, value());
        else if (allow_reads && opt == "--precision-cutoff") a.precision = to_number<double>(opt, value());
        else if (allow_reads && opt == "--phred-cutoff") a.phred_cutoff = to_number<unsigned>(opt, value());
        else if (allow_reads && opt == "--fixed-accuracy") a.fixed_accuracy = to_number<double>(opt, value());
        else if (allow_refs && opt == "--prefix-q") a.prefix_q = to_number<unsigned>(opt, value());
        else if (allow_refs && opt == "--pair-steps") a.pair_steps = to_number<unsigned>(opt, value()) != 0;
        else if (allow_refs && opt == "--label-table") {
            const std::string v = value();
            a.label_table = v == "auto" ? 2u : (to_number<unsigned>(opt, v) != 0 ? 1u : 0u);
        }
        else if (allow_refs && opt == "--triple-steps") {
            const std::string v = value();
            a.triple_steps = v == "auto" ? 2u : (to_number<unsigned>(opt, v) != 0 ? 1u : 0u);
        }
        else if (allow_refs && opt == "--gpu-build") {
            const std::string v = value();
            if (v == "auto") a.gpu_build = -1;
            else a.gpu_build = to_number<unsigned>(opt, v) != 0 ? 1 : 0;
        }
        else if (opt == "--device") a.device = to_number<int>(opt, value());
        else if (allow_reads && opt == "--gpus") a.gpus = (int)to_number<unsigned>(opt, value());
        else if (allow_reads && opt == "--devices") {
            const std::string v = value();
            a.devices.clear();
            for (size_t b = 0; b <= v.size();) {
                size_t e = v.find(',', b);
                if (e == std::string::npos) e = v.size();
                a.devices.push_back((int)to_number<unsigned>(opt, v.substr(b, e - b)));
                b = e + 1;
            }
        }
        else if (allow_reads && opt == "--group-sets") a.out_file_group_sets = value();
        else if (allow_reads && opt == "--marker-coverage") a.out_file_marker_coverage = value();
        else if (allow_reads && opt == "--marker-track") a.out_file_marker_track = value();
        else if (allow_reads && opt == "--track-bin") {
            a.track_bin = to_number<unsigned>(opt, value());
            a.track_bin_given = true;
        }
        else if (allow_reads && opt == "--bootstrap") a.out_file_bootstrap = value();
        else if (allow_reads && opt == "--bootstrap-em") a.out_file_bootstrap_em = value();
        else if (allow_reads && opt == "--bootstrap-replicates") a.bootstrap_replicates = to_number<unsigned>(opt, value());
        else if (allow_reads && opt == "--bootstrap-seed") a.bootstrap_seed = to_number<uint64_t>(opt, value());
        else if (allow_reads && opt == "--bootstrap-level") a.bootstrap_level = to_number<double>(opt, value());
        else if (allow_reads && opt == "--dedup") a.out_file_dedup = value();
        else if (allow_reads && opt == "--max-em-iterations") a.max_em_iterations = to_number<unsigned>(opt, value());
        else throw ParseError("Unknown option " + opt + ". In case this is meant to be a non-option/argument/parameter, "
                              "please specify the start of non-options with '--'.");
    }
    // validators (src/arg_parse.cpp:33-34, :62-63, :101)
    if (a.fixed_accuracy < 0.0 || a.fixed_accuracy > 1.0)
        throw ParseError("Validation failed for option --fixed-accuracy: Value " + std::to_string(a.fixed_accuracy) +
                         " is not in range [0.000000,1.000000].");
    const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
    if (a.threads < 2 || a.threads > hw)
        throw ParseError("Validation failed for option -t/--threads: Value " + std::to_string(a.threads) +
                         " is not in range [2," + std::to_string(hw) + "].");
    if (a.kmer < 1) throw ParseError("Validation failed for option -k/--kmer: must be >= 1");
    if (a.bootstrap_replicates < 1 || a.bootstrap_replicates > SPEQ_BOOTSTRAP_MAX_REPLICATES)
        throw ParseError("Validation failed for option --bootstrap-replicates: Value " +
                         std::to_string(a.bootstrap_replicates) + " is not in range [1," +
                         std::to_string(SPEQ_BOOTSTRAP_MAX_REPLICATES) + "].");
    if (!(a.bootstrap_level > 0.0 && a.bootstrap_level < 1.0))
        throw ParseError("Validation failed for option --bootstrap-level: Value " + std::to_string(a.bootstrap_level) +
                         " is not in range (0,1).");
    if (a.track_bin < 1 || a.track_bin > SPEQ_TRACK_MAX_BIN)
        throw ParseError("Validation failed for option --track-bin: Value " + std::to_string(a.track_bin) +
                         " is not in range [1," + std::to_string(SPEQ_TRACK_MAX_BIN) + "].");
    if (a.track_bin_given && a.out_file_marker_track.empty())
        throw ParseError("Option --track-bin needs --marker-track FILE.");
    if (a.prefix_q > 13) throw ParseError("Validation failed for option --prefix-q: must be <= 13");
    if (a.is_scanner) {
        check_in_file(a.in_file_reads_path_1);
        check_in_file(a.in_file_reads_path_2);
        if (a.in_file_reads_path_1.empty()) throw ParseError("Option -1/--forward is required.");
    }
    if (a.is_indexer) {
        check_in_file(a.in_file_references);
        check_in_file(a.in_file_references_groups);
        if (a.in_file_references.empty() || a.in_file_references_groups.empty())
            throw ParseError("Options -r/--reference and -g/--groups are required.");
    }
    if (a.is_scanner && !a.is_indexer) {
        fs::path idx = a.io_file_index;
        idx.replace_extension(".idx");
        check_in_file(idx);
        a.io_file_index = idx;
    }
    check_out_file(a.out_file_path, a.is_force);
    if (!a.out_file_group_sets.empty()) check_out_file(a.out_file_group_sets, a.is_force);
    if (!a.out_file_marker_coverage.empty()) check_out_file(a.out_file_marker_coverage, a.is_force);
    if (!a.out_file_marker_track.empty()) check_out_file(a.out_file_marker_track, a.is_force);
    if (!a.out_file_bootstrap.empty()) check_out_file(a.out_file_bootstrap, a.is_force);
    if (!a.out_file_bootstrap_em.empty()) check_out_file(a.out_file_bootstrap_em, a.is_force);
    if (!a.out_file_dedup.empty()) check_out_file(a.out_file_dedup, a.is_force);
    a.is_parsed = true;
    return a;
}

void check_in_file(fs::path& p) {
    if (p.empty()) return;
    if (p.is_relative()) {
        if (fs::exists(fs::current_path() / p)) p = fs::current_path() / p;
        else throw ParseError("Validation failed: The relative-path file " + p.string() + " was not found.");
    } else if (!fs::exists(p)) {
        throw ParseError("Validation failed: The full-path file " + p.string() + " was not found.");
    }
}

void check_out_file(fs::path& p, bool is_force) {
    if (p.is_relative()) {
        p = fs::current_path() / p;
        if (fs::exists(p) && !is_force)
            throw ParseError("Validation failed: Cowardly refusing to use an existing output file. Use '-f' to overwrite.");
    }
}

}  // namespace speq::args

// ------------------------------------------------------------------------------------------------------------
namespace {

using speq::args::CmdArguments;

struct CApiError : std::runtime_error {
    explicit CApiError(const std::string& m) : std::runtime_error(m) {}
};

void ok(int rc, const char* what) {
    if (rc != SPEQ_OK) throw CApiError(std::string(what) + ": " + speq_last_error());
}

int64_t mtime_ns(const fs::path& p) {
    return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(fs::last_write_time(p).time_since_epoch()).count();
}

// ---- index header (stored in front of the FM-index; reference: fm_indexer.cpp:39-50) ----
struct IndexHeader {
    std::string ref_path;
    int64_t ref_mtime = 0, groups_mtime = 0;
    std::vector<std::string> names;
    std::vector<int32_t> scaffolds;
    std::vector<int32_t> counts;
};

void put_u64(std::string& s, uint64_t v) { s.append(reinterpret_cast<const char*>(&v), 8); }
void put_str(std::string& s, const std::string& v) { put_u64(s, v.size()); s += v; }
template <typename T>
void put_vec(std::string& s, const std::vector<T>& v) {
    put_u64(s, v.size());
    s.append(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(T));
}

struct Reader {
    const uint8_t* p;
    size_t n, i = 0;
    void need(size_t k) { if (i + k > n) throw CApiError("corrupt index header"); }
    uint64_t u64() { need(8); uint64_t v; std::memcpy(&v, p + i, 8); i += 8; return v; }
    std::string str() { uint64_t l = u64(); need(l); std::string s(reinterpret_cast<const char*>(p + i), l); i += l; return s; }
    template <typename T>
    std::vector<T> vec() {
        uint64_t l = u64();
        need(l * sizeof(T));
        std::vector<T> v(l);
        if (l) std::memcpy(v.data(), p + i, l * sizeof(T));
        i += l * sizeof(T);
        return v;
    }
};

std::string encode_header(const IndexHeader& h) {
    std::string s;
    put_str(s, h.ref_path);
    put_u64(s, (uint64_t)h.ref_mtime);
    put_u64(s, (uint64_t)h.groups_mtime);
    put_u64(s, h.names.size());
    for (auto& n : h.names) put_str(s, n);
    put_vec(s, h.scaffolds);
    put_vec(s, h.counts);
    return s;
}

IndexHeader decode_header(const void* data, uint64_t len) {
    Reader r{static_cast<const uint8_t*>(data), (size_t)len};
    IndexHeader h;
    h.ref_path = r.str();
    h.ref_mtime = (int64_t)r.u64();
    h.groups_mtime = (int64_t)r.u64();
    uint64_t ng = r.u64();
    for (uint64_t i = 0; i < ng; ++i) h.names.push_back(r.str());
    h.scaffolds = r.vec<int32_t>();
    h.counts = r.vec<int32_t>();
    return h;
}

bool read_index_header(const fs::path& p, IndexHeader& h) {
    void* data = nullptr;
    uint64_t len = 0;
    if (speq_index_read_header(p.c_str(), &data, &len) != SPEQ_OK) return false;
    try {
        h = decode_header(data, len);
    } catch (...) {
        speq_free(data);
        return false;
    }
    speq_free(data);
    return true;
}

// ---- speq index (fm_indexer.cpp:55-111) ----
void generate_fm_index(const CmdArguments& a, const fs::path& idx_path, const IndexHeader& h) {
    speq::SeqBatch refs = speq::read_sequences(a.in_file_references.string(), false);
    if (refs.size() == 0) throw CApiError("no sequences in reference file " + a.in_file_references.string());
    int bdev = a.device;
    if (bdev < 0) {
        const char* lr = std::getenv("LOCAL_RANK");
        bdev = lr ? std::atoi(lr) : 0;
    }
    const bool gpu = a.gpu_build == 1 || (a.gpu_build < 0 && speq_device_count() > 0);
    speq_build_opts opts{a.prefix_q, a.threads, a.pair_steps ? 1u : 0u, a.label_table, gpu ? 1u : 0u, bdev,
                         a.pair_steps ? a.triple_steps : 0u};
    speq_index* idx = nullptr;
    ok(speq_index_build(refs.seq.data(), refs.offsets.data(), (uint32_t)refs.size(), h.scaffolds.data(),
                        (uint32_t)h.scaffolds.size(), (uint32_t)h.names.size(), &opts, &idx),
       "building the FM-index");
    const std::string hdr = encode_header(h);
    int rc = speq_index_save(idx, idx_path.c_str(), hdr.data(), hdr.size());
    speq_index_free(idx);
    ok(rc, "writing the index");
}

int run_index(CmdArguments& a) {
    IndexHeader h;
    h.ref_path = a.in_file_references.string();
    h.ref_mtime = mtime_ns(a.in_file_references);
    h.groups_mtime = mtime_ns(a.in_file_references_groups);
    std::string perr;
    speq::Groupings g = speq::parse_groupings(a.in_file_references_groups.string(), &perr);
    if (!perr.empty()) std::cerr << perr;
    h.names = g.names;
    h.scaffolds.assign(g.scaffolds.begin(), g.scaffolds.end());
    h.counts.assign(g.counts.begin(), g.counts.end());
    fs::path idx_path = a.io_file_index;
    idx_path.replace_extension(".idx");  // the reference tests exists() before this (fm_indexer.cpp:68 vs :72)
    IndexHeader old;
    if (fs::exists(idx_path) && !a.is_force && read_index_header(idx_path, old) && old.ref_path == h.ref_path &&
        old.ref_mtime == h.ref_mtime && old.groups_mtime == h.groups_mtime) {
        a.io_file_index = idx_path;
        return 0;  // up to date (fm_indexer.cpp:81-85)
    }
    generate_fm_index(a, idx_path, h);
    a.io_file_index = idx_path;
    return 0;
}

// ---- .dat cache: cereal binary of {file_time_type idx mtime, vector<size_t> unique, vector<size_t> total} ----
fs::path dat_path(const fs::path& idx, unsigned k) {
    fs::path p = idx;
    p.replace_filename(idx.stem().string() + "_" + std::to_string(k) + "mer.dat");
    return p;
}

bool read_dat(const fs::path& p, int64_t idx_mtime, size_t G, std::vector<uint64_t>& u, std::vector<uint64_t>& t) {
    std::ifstream is(p, std::ios::binary);
    if (!is) return false;
    int64_t stamp = 0;
    uint64_t n1 = 0, n2 = 0;
    is.read(reinterpret_cast<char*>(&stamp), 8);
    if (!is || stamp != idx_mtime) return false;
    is.read(reinterpret_cast<char*>(&n1), 8);
    if (!is || n1 != G) return false;
    u.resize(G);
    is.read(reinterpret_cast<char*>(u.data()), (std::streamsize)(8 * G));
    is.read(reinterpret_cast<char*>(&n2), 8);
    if (!is || n2 != G) return false;
    t.resize(G);
    is.read(reinterpret_cast<char*>(t.data()), (std::streamsize)(8 * G));
    return (bool)is;
}

void write_dat(const fs::path& p, int64_t idx_mtime, const std::vector<uint64_t>& u, const std::vector<uint64_t>& t) {
    std::ofstream os(p, std::ios::binary | std::ios::trunc);
    if (!os) throw CApiError("cannot write " + p.string());
    uint64_t G = u.size();
    os.write(reinterpret_cast<const char*>(&idx_mtime), 8);
    os.write(reinterpret_cast<const char*>(&G), 8);
    os.write(reinterpret_cast<const char*>(u.data()), (std::streamsize)(8 * G));
    os.write(reinterpret_cast<const char*>(&G), 8);
    os.write(reinterpret_cast<const char*>(t.data()), (std::streamsize)(8 * G));
}

// unique_to_percent (fm_scanner.cpp:1455-1474)
std::vector<double> unique_to_percent(const std::vector<double>& ur, uint64_t total, const std::vector<double>& uref,
                                      const std::vector<double>& tref) {
    std::vector<double> out(uref.size(), 0.0);
    for (size_t i = 0; i < uref.size(); ++i) {
        if (tref[i] > 0.0) {
            const double pu = uref[i] / tref[i];
            out[i] = 100.0 * ur[i] / static_cast<double>(total) / pu;
        }
    }
    return out;
}

std::vector<double> to_double(const std::vector<uint64_t>& v) { return std::vector<double>(v.begin(), v.end()); }

// ---- speq scan (fm_scanner.cpp:5-32 and the four mode variants) ----
// SPEQ_CLI_TIMING=1: wall seconds of each scan phase on stderr (performance investigation only).
struct PhaseClock {
    bool on = false;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    PhaseClock() {
        const char* v = std::getenv("SPEQ_CLI_TIMING");
        on = v && *v && *v != '0';
        since_launch("launch -> main");
    }
    // SPEQ_T0 (ns since the epoch, set by a timing harness just before it starts the process): process start-up cost
    void since_launch(const char* what) const {
        const char* t0 = std::getenv("SPEQ_T0");
        if (!on || !t0 || !*t0) return;
        const double now = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
        std::fprintf(stderr, "speq: %-22s %.4f s\n", what, now - std::strtod(t0, nullptr) * 1e-9);
    }
    void operator()(const char* what) {
        const auto now = std::chrono::steady_clock::now();
        if (on) std::fprintf(stderr, "speq: %-22s %.4f s\n", what, std::chrono::duration<double>(now - t).count());
        t = now;
    }
};

// ---- one process per GPU (RANK / WORLD_SIZE / LOCAL_RANK from a launcher such as `torchrun --no-python`) ----
// Every rank opens its own replica on GPU $LOCAL_RANK, scans its share of the FASTQ blocks and of the reference
// windows, and the sums are all-reduces (speq_allreduce_host / speq_em_allreduce): the reference's future.get()
// sums (fm_scanner.cpp:224-233) across processes. Rank 0 prints and writes everything; the others print nothing.
// The ranks meet through speq_comm_connect: rank 0 publishes {nonce, port} in a rendezvous file ($SPEQ_RENDEZVOUS,
// default /tmp/speq_rdzv_<parent pid>_<MASTER_PORT>_<TORCHELASTIC_RUN_ID>: the launcher is every rank's parent) only
// after its index step, so `speq all` ranks also wait for the index there. The transport is RCCL when the ranks are
// on different GPUs, host sockets when they share one ($SPEQ_COMM = rccl | host forces it).
struct Dist {
    int rank = 0, world = 1, device = 0;
    void* comm = nullptr;
    bool on() const { return world > 1; }
};

int env_int(const char* name, int dflt) {
    const char* v = std::getenv(name);
    return v && *v ? std::atoi(v) : dflt;
}

Dist dist_from_env(const CmdArguments& a) {
    Dist dd;
    const int world = env_int("WORLD_SIZE", 1);
    if (world <= 1 || !a.devices.empty() || a.gpus != 1) return dd;
    dd.world = world;
    dd.rank = env_int("RANK", 0);
    dd.device = a.device >= 0 ? a.device : env_int("LOCAL_RANK", 0);
    if (dd.rank < 0 || dd.rank >= world) throw CApiError("RANK " + std::to_string(dd.rank) + " outside WORLD_SIZE");
    return dd;
}

std::string rendezvous_path() {
    if (const char* v = std::getenv("SPEQ_RENDEZVOUS"); v && *v) return v;
    const char* port = std::getenv("MASTER_PORT");
    const char* run = std::getenv("TORCHELASTIC_RUN_ID");
    const char* tmp = std::getenv("TMPDIR");
    return std::string(tmp && *tmp ? tmp : "/tmp") + "/speq_rdzv_" + std::to_string((long)getppid()) + "_" +
           (port ? port : "0") + "_" + (run && *run ? run : "none");
}

// Rank 0 of a one-process-per-GPU run clears a rendezvous file left by an earlier, crashed run before its (possibly
// long) index step; the other ranks would skip it anyway (its nonce and port are dead).
void dist_clear_stale(const Dist& dd) {
    if (dd.on() && dd.rank == 0) {
        std::error_code ec;
        fs::remove(rendezvous_path(), ec);
    }
}

void dist_connect(Dist& dd) {
    int transport = SPEQ_COMM_AUTO;
    if (const char* v = std::getenv("SPEQ_COMM"); v && *v) {
        const std::string t(v);
        if (t == "rccl") transport = SPEQ_COMM_RCCL;
        else if (t == "host") transport = SPEQ_COMM_HOST;
        else if (t != "auto") throw CApiError("SPEQ_COMM must be auto, rccl or host");
    }
    const int limit_s = env_int("SPEQ_RENDEZVOUS_TIMEOUT", 600);
    ok(speq_comm_connect(dd.world, dd.rank, dd.device, rendezvous_path().c_str(), transport, limit_s, &dd.comm),
       "joining the ranks");
}

// Sums u64 (or f64) words over the ranks, in place.
void dist_sum(const Dist& dd, void* buf, size_t n, bool f64) {
    if (dd.on() && n) ok(speq_allreduce_host(dd.comm, dd.device, buf, n, f64 ? 1 : 0), "all-reduce over ranks");
}

// FILE of --group-sets: "units<TAB>n_groups<TAB>name1,name2,..." per distinct group set, ascending by the set read as
// one integer (the empty set, "-", first).
void write_group_sets(const CmdArguments& a, speq_device_index* d, const speq_scan_params& prm,
                      const std::vector<std::string>& names) {
    speq_group_sets* gs = nullptr;
    ok(speq_report_fastq(d, a.in_file_reads_path_1.c_str(),
                         a.in_file_reads_path_2.empty() ? nullptr : a.in_file_reads_path_2.c_str(), &prm, a.threads, &gs,
                         nullptr),
       "reporting group sets");
    std::unique_ptr<speq_group_sets, void (*)(speq_group_sets*)> guard(gs, speq_group_sets_free);
    std::ofstream of(a.out_file_group_sets);
    if (!of) throw CApiError("cannot write " + a.out_file_group_sets.string());
    std::vector<uint64_t> words(SPEQ_SET_WORDS(names.size()));
    const uint64_t n = speq_group_sets_count(gs);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t units = 0;
        ok(speq_group_sets_get(gs, i, words.data(), &units), "reading group sets");
        std::string list;
        size_t n_groups = 0;
        for (size_t g = 0; g < names.size(); ++g)
            if ((words[g / 64] >> (g % 64)) & 1u) {
                if (n_groups++) list += ",";
                list += names[g];
            }
        of << units << "\t" << n_groups << "\t" << (n_groups ? list : std::string("-")) << "\n";
    }
}

// FILE of --marker-coverage: a header line, then per group (groupings order) its name, markers, observed,
// breadth = observed / markers, hits, mean_depth = hits / markers, expected_breadth = 1 - exp(-mean_depth) (the breadth
// uniform sampling at that depth would give), max_depth and the eight depth bins; the ratios are "-" without markers.
//
// FILE of --marker-track: a header line, then per record (FASTA order) one line per bin of --track-bin loci: the
// record's number, its group's name, the bin's first locus and one past its last, markers, observed, breadth, hits,
// mean_depth, max_depth. When both files are asked for, one pass over the reads serves both.
struct MarkerTrackRows {
    std::vector<uint64_t> first_bin;  // [R + 1]
    speq_marker_bin* rows = nullptr;  // the library's, freed with speq_free
    ~MarkerTrackRows() { speq_free(rows); }
};

std::string ratio6(double x) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.6f", x);
    return std::string(buf);
}

void write_marker_track(const CmdArguments& a, const speq_index* idx, const MarkerTrackRows& t,
                        const std::vector<std::string>& names) {
    const void* tg = nullptr;
    uint64_t tg_bytes = 0, nwin_total = 0;
    ok(speq_index_array(idx, "text_group", &tg, &tg_bytes), "reading the index");
    const int32_t* text_group = static_cast<const int32_t*>(tg);
    const uint32_t n_rec = (uint32_t)(t.first_bin.size() - 1);
    std::vector<uint64_t> first_locus(n_rec + 1);  // the layout at bin 1: the loci per record
    ok(speq_index_track_layout(idx, a.kmer, 1, &nwin_total, first_locus.data()), "marker track");
    std::ofstream of(a.out_file_marker_track);
    if (!of) throw CApiError("cannot write " + a.out_file_marker_track.string());
    of << "record\tgroup\tstart\tend\tmarkers\tobserved\tbreadth\thits\tmean_depth\tmax_depth\n";
    for (uint32_t r = 0; r < n_rec; ++r) {
        const uint64_t loci = first_locus[r + 1] - first_locus[r];
        const std::string& group = names[(size_t)text_group[2 * (size_t)r]];
        for (uint64_t i = t.first_bin[r]; i < t.first_bin[r + 1]; ++i) {
            const speq_marker_bin& c = t.rows[i];
            const uint64_t start = (i - t.first_bin[r]) * a.track_bin;
            const bool has = c.markers > 0;
            of << r << "\t" << group << "\t" << start << "\t" << std::min<uint64_t>(start + a.track_bin, loci) << "\t"
               << c.markers << "\t" << c.observed << "\t"
               << (has ? ratio6((double)c.observed / (double)c.markers) : std::string("-")) << "\t" << c.hits << "\t"
               << (has ? ratio6((double)c.hits / (double)c.markers) : std::string("-")) << "\t" << c.max_depth << "\n";
        }
    }
}

void write_marker_coverage(const CmdArguments& a, const speq_index* idx, speq_device_index* d,
                           const speq_scan_params& prm, const std::vector<std::string>& names, MarkerTrackRows* track) {
    std::vector<speq_marker_cov> cov(names.size());
    const char* p1 = a.in_file_reads_path_1.c_str();
    const char* p2 = a.in_file_reads_path_2.empty() ? nullptr : a.in_file_reads_path_2.c_str();
    if (track) {
        speq_index_info info{};
        ok(speq_index_get_info(idx, &info), "reading the index");
        track->first_bin.assign((size_t)info.n_records + 1, 0);
        uint64_t n_bins = 0;
        ok(speq_markers_track_fastq(d, p1, p2, &prm, a.threads, a.track_bin,
                                    a.out_file_marker_coverage.empty() ? nullptr : cov.data(), track->first_bin.data(),
                                    &track->rows, &n_bins, nullptr),
           "marker track");
    } else {
        ok(speq_markers_fastq(d, p1, p2, &prm, a.threads, cov.data(), nullptr), "marker coverage");
    }
    if (a.out_file_marker_coverage.empty()) return;
    std::ofstream of(a.out_file_marker_coverage);
    if (!of) throw CApiError("cannot write " + a.out_file_marker_coverage.string());
    of << "name\tmarkers\tobserved\tbreadth\thits\tmean_depth\texpected_breadth\tmax_depth";
    for (int j = 0; j < SPEQ_MARKER_BINS; ++j) of << "\td" << j;
    of << "\n";
    auto ratio = [](double x) {
        char buf[64];
        std::snprintf(buf, sizeof buf, "%.6f", x);
        return std::string(buf);
    };
    for (size_t g = 0; g < names.size(); ++g) {
        const speq_marker_cov& c = cov[g];
        const bool has = c.markers > 0;
        const double mean = has ? (double)c.hits / (double)c.markers : 0.0;
        of << names[g] << "\t" << c.markers << "\t" << c.observed << "\t"
           << (has ? ratio((double)c.observed / (double)c.markers) : std::string("-")) << "\t" << c.hits << "\t"
           << (has ? ratio(mean) : std::string("-")) << "\t" << (has ? ratio(1.0 - std::exp(-mean)) : std::string("-"))
           << "\t" << c.max_depth;
        for (int j = 0; j < SPEQ_MARKER_BINS; ++j) of << "\t" << c.depth_hist[j];
        of << "\n";
    }
}

// FILE of --bootstrap: a header line, then per group (groupings order) its name, the run's initial percentage, and over
// the replicates' percentages their mean, standard deviation (the bootstrap standard error), the lo and hi order
// statistics of the level, and how many replicates had a passing window at all. FILE of --bootstrap-em: the same
// columns for the EM-refined percentages, `percent` being the run's own refined vector (the one written to -o). One
// pass over the reads serves both files; with --bootstrap-em the finalized histogram `em` of the run is attached, so
// that the pass fills one histogram per replicate, and every replicate is refined by the run's own loop.
void write_table(const fs::path& path, const std::vector<std::string>& names, const std::vector<speq_bootstrap_ci>& ci) {
    std::ofstream of(path);
    if (!of) throw CApiError("cannot write " + path.string());
    of << "name\tpercent\tmean\tse\tlo\thi\tused\n";
    for (size_t g = 0; g < names.size(); ++g) {
        char buf[400];
        std::snprintf(buf, sizeof buf, "\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%llu\n", ci[g].estimate, ci[g].mean, ci[g].se,
                      ci[g].lo, ci[g].hi, (unsigned long long)ci[g].used);
        of << names[g] << buf;
    }
}

void write_bootstrap(const CmdArguments& a, speq_device_index* d, const speq_scan_params& prm,
                     const std::vector<std::string>& names, const std::vector<uint64_t>& u_ref,
                     const std::vector<uint64_t>& tot_ref, const speq_em* em, const std::vector<int32_t>& group_counts,
                     const std::vector<double>& refined) {
    const size_t G = names.size();
    const uint32_t B = a.bootstrap_replicates;
    const bool local = prm.mode == SPEQ_MODE_LOCAL;
    const bool with_em = !a.out_file_bootstrap_em.empty();
    std::vector<uint64_t> counts((size_t)(B + 1) * (G + 2), 0);
    std::vector<double> weights(local ? std::max<size_t>((size_t)(B + 1) * G, 1) : 0, 0.0);
    const char* p1 = a.in_file_reads_path_1.c_str();
    const char* p2 = a.in_file_reads_path_2.empty() ? nullptr : a.in_file_reads_path_2.c_str();
    uint64_t n_rows = 0, n_entries = 0, missed = 0;
    std::vector<uint64_t> mult;
    if (with_em) {
        ok(speq_em_rows(em, &n_rows, &n_entries, nullptr, nullptr, nullptr, nullptr), "reading the EM histogram");
        mult.assign(std::max<size_t>((size_t)(B + 1) * n_rows, 1), 0);
        ok(speq_bootstrap_em_fastq(d, em, p1, p2, &prm, B, a.bootstrap_seed, a.threads, counts.data(),
                                   local ? weights.data() : nullptr, mult.data(), &missed, nullptr),
           "bootstrapping the reads");
        if (missed != 0)
            throw CApiError("bootstrapping the reads: " + std::to_string(missed) +
                            " windows lie in intervals that the scan's EM histogram does not hold");
    } else {
        ok(speq_bootstrap_fastq(d, p1, p2, &prm, B, a.bootstrap_seed, a.threads, counts.data(),
                                local ? weights.data() : nullptr, nullptr),
           "bootstrapping the reads");
    }
    std::vector<speq_bootstrap_ci> ci(std::max<size_t>(G, 1));
    const double scale = local ? 1.0 : 1.0 / std::pow(a.fixed_accuracy, (double)a.kmer);
    if (!a.out_file_bootstrap.empty()) {
        ok(speq_bootstrap_summary(counts.data(), local ? weights.data() : nullptr, B, (uint32_t)G, u_ref.data(),
                                  tot_ref.data(), scale, a.bootstrap_level, ci.data()),
           "summarising the bootstrap");
        write_table(a.out_file_bootstrap, names, ci);
    }
    if (!with_em) return;
    std::vector<uint64_t> row_ptr(n_rows + 1, 0);
    std::vector<uint32_t> grp(std::max<uint64_t>(n_entries, 1)), cnt(std::max<uint64_t>(n_entries, 1));
    ok(speq_em_rows(em, nullptr, nullptr, nullptr, row_ptr.data(), grp.data(), cnt.data()), "reading the EM histogram");
    std::vector<double> percent(std::max<size_t>((size_t)(B + 1) * G, 1), 0.0);
    std::vector<uint32_t> iterations(B + 1, 0);
    ok(speq_em_rows_refine((uint32_t)G, n_rows, row_ptr.data(), grp.data(), cnt.data(), B, mult.data(), counts.data(),
                           local ? weights.data() : nullptr, scale, u_ref.data(), tot_ref.data(), group_counts.data(),
                           a.precision, a.max_em_iterations, percent.data(), iterations.data()),
       "refining the replicates");
    std::vector<uint8_t> used(B + 1, 0);
    uint32_t stopped = 0;
    for (uint32_t b = 0; b <= B; ++b) {
        used[b] = counts[(size_t)b * (G + 2)] != 0;
        if (b && used[b] && iterations[b] >= a.max_em_iterations) ++stopped;
    }
    if (stopped)
        std::cerr << "speq: the EM of " << stopped << " of " << B
                  << " bootstrap replicates ran --max-em-iterations steps\n";
    ok(speq_bootstrap_summary_percent(percent.data(), refined.data(), used.data(), B, (uint32_t)G, a.bootstrap_level,
                                      ci.data()),
       "summarising the bootstrap");
    write_table(a.out_file_bootstrap_em, names, ci);
}

// The refinement loop of `speq scan` (fm_scanner.cpp:248-279, :515-545, :761-792, :1035-1065) over a finalized
// histogram: steps until the largest change of a percentage is within --precision-cutoff, or --max-em-iterations steps
// were made. `print`: the run's own refinement writes what the reference writes to stderr per step; --dedup's runs the
// same loop on the deduplicated counters and prints nothing.
std::vector<double> refine_percentages(const CmdArguments& a, const speq_em* em, std::vector<double> percent,
                                       const std::vector<double>& unique_totals, uint64_t total,
                                       const std::vector<uint64_t>& unique, const std::vector<int32_t>& group_counts,
                                       bool local, bool paired, bool print) {
    const size_t G = percent.size();
    std::vector<double> diff(G, 1.0), next(G);
    for (unsigned it = 0; G > 0 && *std::max_element(diff.begin(), diff.end()) > a.precision; ++it) {
        if (it >= a.max_em_iterations) {
            if (print) std::cerr << "speq: EM stopped after " << it << " iterations (--max-em-iterations)\n";
            break;
        }
        ok(speq_em_step(em, percent.data(), group_counts.data(), unique.data(), next.data()), "EM step");
        if (print && local && !paired)
            std::cerr << "1: " << speq::format_vector(unique_totals) << "\n2: " << total << "\n3: "
                      << speq::format_vector(next) << "\n";
        std::vector<double> np = unique_to_percent(unique_totals, total, unique_totals, next);
        for (size_t i = 0; i < G; ++i) diff[i] = std::fabs(np[i] - percent[i]);
        percent = np;
        if (!print) continue;
        if (local && !paired) {
            std::cerr << "Percent of each group: " << speq::format_vector(percent) << "\n";
            std::cerr << "Total Kmers per group: " << speq::format_vector(next) << "\n\n";
        } else {
            std::cerr << speq::format_vector(percent) << "\n" << speq::format_vector(next) << "\n\n";
        }
    }
    return percent;
}

// FILE of --dedup: '#' lines with the duplicate statistics, a header line, then per group (groupings order) its name,
// the run's initial and refined percentages, and the same two from the reads with every distinct read (pair) counted
// once. The deduplicated scan fills a histogram of its own, which the run's own refinement loop then refines.
void write_dedup(const CmdArguments& a, const speq_index* idx, speq_device_index* d, const speq_scan_params& prm,
                 const std::vector<std::string>& names, const std::vector<uint64_t>& u_ref,
                 const std::vector<uint64_t>& tot_ref, const std::vector<int32_t>& group_counts,
                 const std::vector<double>& initial, const std::vector<double>& refined) {
    const size_t G = names.size();
    const bool local = prm.mode == SPEQ_MODE_LOCAL, paired = prm.paired != 0;
    speq_em* em = nullptr;
    ok(speq_em_create(idx, d, &em), "allocating the EM histogram");
    struct Free {
        speq_em* e;
        ~Free() { speq_em_free(e); }
    } free_em{em};
    std::vector<uint64_t> counts(G + 2, 0);
    std::vector<double> weights(std::max<size_t>(G, 1), 0.0);
    speq_dedup_stats ds{};
    ok(speq_dedup_fastq(d, em, a.in_file_reads_path_1.c_str(),
                        a.in_file_reads_path_2.empty() ? nullptr : a.in_file_reads_path_2.c_str(), &prm, a.threads, &ds,
                        counts.data(), local ? weights.data() : nullptr, nullptr),
       "deduplicating the reads");
    ok(speq_em_finalize(em, a.threads), "building the EM histogram");
    const uint64_t total = counts[0];
    std::vector<double> unique_totals(G, 0.0);
    if (local) {
        unique_totals.assign(weights.begin(), weights.begin() + G);
    } else {
        const double percent_perfect = std::pow(a.fixed_accuracy, (double)a.kmer);
        for (size_t i = 0; i < G; ++i) unique_totals[i] = static_cast<double>(counts[2 + i]) / percent_perfect;
    }
    const std::vector<double> first = unique_to_percent(unique_totals, total, to_double(u_ref), to_double(tot_ref));
    const std::vector<uint64_t> unique(counts.begin() + 2, counts.end());
    const std::vector<double> last =
        refine_percentages(a, em, first, unique_totals, total, unique, group_counts, local, paired, false);
    std::ofstream of(a.out_file_dedup);
    if (!of) throw CApiError("cannot write " + a.out_file_dedup.string());
    char buf[400];
    std::snprintf(buf, sizeof buf, "%.6f", ds.units ? (double)(ds.units - ds.distinct) / (double)ds.units : 0.0);
    of << "# units " << ds.units << "\n# distinct " << ds.distinct << "\n# duplicates " << ds.units - ds.distinct
       << "\n# duplicate_fraction " << buf << "\n# max_multiplicity " << ds.max_multiplicity
       << "\n# multiplicity_hist";
    for (int j = 0; j < SPEQ_DEDUP_BINS; ++j) of << " " << ds.mult_hist[j];
    of << "\nname\tpercent\tpercent_dedup\trefined\trefined_dedup\n";
    for (size_t g = 0; g < G; ++g) {
        std::snprintf(buf, sizeof buf, "\t%.6f\t%.6f\t%.6f\t%.6f\n", initial[g], first[g], refined[g], last[g]);
        of << names[g] << buf;
    }
}

int run_scan(CmdArguments& a) {
    PhaseClock phase;
    Dist dd = dist_from_env(a);
    if (dd.on()) {
        dist_connect(dd);
        phase("rendezvous");
    }
    // GPUs: --devices list, --gpus N (0..N-1), or one (--device, $LOCAL_RANK, 0). Reads shard across them in-process
    // (SURVEY 8(e)): one replica of the index per GPU, the counters summed at the end.
    std::vector<int> devs = a.devices;
    if (dd.on()) devs = {dd.device};
    if (devs.empty() && a.gpus != 1) {
        const int visible = speq_device_count();
        const int n = a.gpus == 0 ? visible : a.gpus;
        if (n < 1 || n > visible)
            throw CApiError("--gpus " + std::to_string(a.gpus) + ": " + std::to_string(visible) + " GPU(s) visible");
        for (int i = 0; i < n; ++i) devs.push_back(i);
    }
    if (devs.empty()) {
        int dev = a.device;
        if (dev < 0) {
            const char* lr = std::getenv("LOCAL_RANK");
            dev = lr ? std::atoi(lr) : 0;
        }
        devs.push_back(dev);
    }
    const uint32_t n_dev = (uint32_t)devs.size();
    const bool paired = !a.in_file_reads_path_2.empty();
    // While the index loads: the HIP runtime, each GPU's context, the library's GPU code and ready streams
    // (speq_device_warmup), and with one GPU per process the FASTQ stream's pinned and device slot buffers
    // (speq_stream_reserve) — all of it had been on the critical path after the load (~0.2 s of a config-3 scan,
    // profiles/r06/cli_trace_*). Failures here are left to speq_device_open / the stream to report.
    // (device open needs only the runtime: it runs beside what is left of the warm-up, joined before the stream)
    std::vector<std::thread> warm;
    // (7 streams: the replica's, the FASTQ stream's copy stream and its 5 compute lanes, set below)
    for (int dv : devs) {
        warm.emplace_back([dv] { (void)speq_device_warmup(dv, 7); });
        if (n_dev == 1) warm.emplace_back([dv, paired, threads = a.threads] { (void)speq_stream_reserve(dv, threads, paired); });
    }
    struct Joiner {
        std::vector<std::thread>& ts;
        ~Joiner() {
            for (auto& t : ts)
                if (t.joinable()) t.join();
        }
    } join_warm{warm};
    fs::path idx_path = a.io_file_index;
    idx_path.replace_extension(".idx");
    speq_index* idx = nullptr;
    void* hdr_data = nullptr;
    uint64_t hdr_len = 0;
    ok(speq_index_load(idx_path.c_str(), &idx, &hdr_data, &hdr_len), "loading the index");
    IndexHeader h = decode_header(hdr_data, hdr_len);
    speq_free(hdr_data);
    const size_t G = h.names.size();
    phase("index load");
    std::vector<speq_device_index*> ds(n_dev, nullptr);
    {  // replicas are uploaded concurrently (one host thread per GPU)
        std::vector<int> rcs(n_dev, SPEQ_OK);
        std::vector<std::string> msgs(n_dev);
        std::vector<std::thread> ts;
        for (uint32_t i = 0; i < n_dev; ++i)
            ts.emplace_back([&, i] {
                rcs[i] = speq_device_open(idx, devs[i], &ds[i]);
                if (rcs[i] != SPEQ_OK) msgs[i] = speq_last_error();
            });
        for (auto& t : ts) t.join();
        for (uint32_t i = 0; i < n_dev; ++i)
            if (rcs[i] != SPEQ_OK) throw CApiError("opening GPU " + std::to_string(devs[i]) + ": " + msgs[i]);
    }
    speq_device_index* d = ds[0];
    // A whole FASTQ file keeps more blocks in flight than the library default's 3 compute lanes carry: config 3's
    // 3.16 GB stream takes 0.127-0.134 s with 4-5 lanes against 0.145-0.147 s with 3 (profiles/r06/cli/lanes.txt;
    // the bench's 316 MB fastq_e2e is within noise of 3 either way)
    for (speq_device_index* x : ds) ok(speq_device_set_tuning(x, "stream_lanes", 5), "setting the stream lanes");
    // SPEQ_TUNE="key=value,..." (performance investigation only): launch tunings of every replica
    // (speq_device_set_tuning; results never depend on them)
    if (const char* tv = std::getenv("SPEQ_TUNE"); tv && *tv) {
        std::string spec(tv);
        size_t at = 0;
        while (at < spec.size()) {
            const size_t end = std::min(spec.find(',', at), spec.size());
            const std::string kv = spec.substr(at, end - at);
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) throw CApiError("SPEQ_TUNE: expected key=value, got '" + kv + "'");
            for (speq_device_index* x : ds)
                ok(speq_device_set_tuning(x, kv.substr(0, eq).c_str(), std::stoll(kv.substr(eq + 1))), "SPEQ_TUNE");
            at = end + 1;
        }
    }
    phase("device open");
    for (auto& t : warm) t.join();
    phase("GPU warm-up (rest)");

    // Reference uniqueness per group, cached in <stem>_<k>mer.dat keyed by the index mtime.
    const int64_t idx_mtime = mtime_ns(idx_path);
    const fs::path dat = dat_path(idx_path, a.kmer);
    std::vector<uint64_t> u_ref, tot_ref;
    uint64_t have_dat = (!dd.on() || dd.rank == 0) && read_dat(dat, idx_mtime, G, u_ref, tot_ref) ? 1 : 0;
    dist_sum(dd, &have_dat, 1, false);  // rank 0's cache decides for every rank
    if (!have_dat) {
        u_ref.assign(G, 0);
        tot_ref.assign(G, 0);
        if (dd.on()) {
            ok(speq_ref_unique_shard(d, a.kmer, (uint32_t)dd.rank, (uint32_t)dd.world, u_ref.data(), tot_ref.data()),
               "reference-uniqueness pass");
            dist_sum(dd, u_ref.data(), G, false);
            dist_sum(dd, tot_ref.data(), G, false);
        } else {
            ok(n_dev == 1 ? speq_ref_unique(d, a.kmer, u_ref.data(), tot_ref.data())
                          : speq_ref_unique_multi(ds.data(), n_dev, a.kmer, u_ref.data(), tot_ref.data()),
               "reference-uniqueness pass");
        }
        if (dd.rank == 0) {
            write_dat(dat, idx_mtime, u_ref, tot_ref);
            std::cerr << speq::format_vector(u_ref) << "\n" << speq::format_vector(tot_ref) << "\n";  // :1572-1573
        }
    }
    phase(".dat");

    const bool local = a.fixed_accuracy == 0.0;
    speq_scan_params prm{a.kmer, a.phred_cutoff, paired ? 1u : 0u, local ? (uint32_t)SPEQ_MODE_LOCAL : (uint32_t)SPEQ_MODE_GLOBAL};
    std::vector<uint64_t> counts(G + 2, 0);
    std::vector<double> weights(std::max<size_t>(G, 1), 0.0);
    // One scan also fills the EM histogram (the reference re-scans every read per EM iteration instead).
    std::vector<speq_em*> ems(n_dev, nullptr);
    for (uint32_t i = 0; i < n_dev; ++i) ok(speq_em_create(idx, ds[i], &ems[i]), "allocating the EM histogram");
    speq_em* em = ems[0];
    phase("EM histogram alloc");
    // FASTQ(.gz) streamed through pinned slots: -t parser threads, H2D overlapped with the kernel (fm_scanner.cpp:
    // 138-141 / :651-655 read through an async_input_buffer; paired files are zipped, stopping at the shorter one).
    speq_stream_stats st{};
    if (dd.on()) {
        // this rank's blocks; the parallel cut unless SPEQ_SPLIT_CUT=0, and when it does not fit the input on ANY
        // rank, every rank scans again with the sequential cutter (same blocks everywhere)
        const char* sc = std::getenv("SPEQ_SPLIT_CUT");
        int cut = sc && sc[0] == '0' ? 0 : 1;
        for (;;) {
            const int rc = speq_scan_fastq_shard(d, em, a.in_file_reads_path_1.c_str(),
                                                 paired ? a.in_file_reads_path_2.c_str() : nullptr, &prm, a.threads,
                                                 (uint32_t)dd.rank, (uint32_t)dd.world, cut, counts.data(),
                                                 local ? weights.data() : nullptr, &st);
            const std::string msg = rc == SPEQ_OK ? "" : speq_last_error();
            uint64_t flags[2] = {rc != SPEQ_OK && rc != SPEQ_E_RETRY ? 1u : 0u, rc == SPEQ_E_RETRY ? 1u : 0u};
            dist_sum(dd, flags, 2, false);
            if (flags[0]) {
                if (rc != SPEQ_OK && rc != SPEQ_E_RETRY) ok(rc, "scanning reads");
                throw CApiError("scanning reads: another rank failed");
            }
            if (!flags[1]) break;
            cut = 0;  // the histogram of a rank whose parallel scan went through is rebuilt from scratch
            speq_em_free(em);
            em = ems[0] = nullptr;
            ok(speq_em_create(idx, d, &em), "allocating the EM histogram");
            ems[0] = em;
        }
        dist_sum(dd, counts.data(), counts.size(), false);
        if (local) dist_sum(dd, weights.data(), G, true);
        uint64_t sv[3] = {st.records, st.bases, st.batches};
        dist_sum(dd, sv, 3, false);
        st.records = sv[0];
        st.bases = sv[1];
        st.batches = sv[2];
        ok(speq_em_allreduce(em, dd.comm, nullptr), "summing the EM histograms over ranks");
        speq_comm_destroy(dd.comm);
        dd.comm = nullptr;
        if (dd.rank != 0) {  // rank 0 refines, prints and writes
            speq_em_free(em);
            return 1;
        }
    } else {
        ok(speq_scan_fastq_multi(ds.data(), ems.data(), n_dev, a.in_file_reads_path_1.c_str(),
                                 paired ? a.in_file_reads_path_2.c_str() : nullptr, &prm, a.threads, counts.data(),
                                 local ? weights.data() : nullptr, &st),
           "scanning reads");
    }
    phase("FASTQ stream + scan");
    if (const char* v = std::getenv("SPEQ_STREAM_STATS"); v && *v && *v != '0')
        std::fprintf(stderr, "speq: streamed %llu records, %llu bases in %llu batches, %.3f s (%.1f M records/s)\n",
                     (unsigned long long)st.records, (unsigned long long)st.bases, (unsigned long long)st.batches,
                     st.seconds, st.seconds > 0 ? st.records / st.seconds / 1e6 : 0.0);
    const uint64_t total = counts[0], ambiguous = counts[1];
    std::vector<double> unique_totals(G, 0.0);
    if (local) {
        unique_totals.assign(weights.begin(), weights.begin() + G);
    } else {
        const double percent_perfect = std::pow(a.fixed_accuracy, (double)a.kmer);  // fm_scanner.cpp:15
        for (size_t i = 0; i < G; ++i) unique_totals[i] = static_cast<double>(counts[2 + i]) / percent_perfect;
    }
    std::vector<double> percent = unique_to_percent(unique_totals, total, to_double(u_ref), to_double(tot_ref));

    // stderr output of the reference (fm_scanner.cpp:245-247, :513-514, :757-759, :1030-1033)
    std::cerr << speq::format_vector(percent) << "\n";
    if (!(local && !paired)) std::cerr << speq::format_vector(unique_totals) << "\n";
    std::cerr << total << "\t" << ambiguous << "\n";
    // Fusion map (paired Phred mode, :915-1033): do_a_count takes set_groups BY VALUE (:916), so every key is the
    // empty set and the map is {{} -> ambiguous pairs}, or empty; seqan3's debug_stream prints a map as a range of
    // (key,value) tuples and a set as a range: "[([],N)]" or "[]".
    if (local && paired) {
        if (ambiguous) std::cerr << "[([]," << ambiguous << ")]\n";
        else std::cerr << "[]\n";
    }

    // EM refinement (fm_scanner.cpp:248-279, :515-545, :761-792, :1035-1065) over the histogram.
    for (uint32_t i = 1; i < n_dev; ++i) {
        ok(speq_em_merge(em, ems[i]), "merging the EM histograms");
        speq_em_free(ems[i]);
    }
    ok(speq_em_finalize(em, a.threads), "building the EM histogram");
    phase("EM finalize");
    if (phase.on) {
        uint64_t rows = 0, ents = 0, wins = 0;
        if (speq_em_info(em, &rows, &ents, &wins) == SPEQ_OK)
            std::fprintf(stderr, "speq: EM histogram: %llu intervals, %llu (group, count) entries, %llu windows\n",
                         (unsigned long long)rows, (unsigned long long)ents, (unsigned long long)wins);
    }
    const std::vector<double> initial = percent;  // the first vector printed above (--dedup's `percent` column)
    std::vector<uint64_t> unique(counts.begin() + 2, counts.end());
    percent = refine_percentages(a, em, percent, unique_totals, total, unique, h.counts, local, paired, true);
    phase("EM iterations");

    // The reference writes nothing to -o (quirk B1); we write the (refined) percentage vector there.
    {
        std::ofstream of(a.out_file_path);
        if (!of) throw CApiError("cannot write " + a.out_file_path.string());
        for (size_t i = 0; i < G; ++i) of << h.names[i] << "\t" << percent[i] << "\n";
    }
    // --group-sets: one report pass over the same reads on the first replica (rank 0 of a one-process-per-GPU run),
    // after everything the run prints and writes otherwise. The degenerate fusion-map line above stays as the
    // reference prints it; this file is the map it meant: the lines of two or more groups.
    if (!a.out_file_group_sets.empty()) {
        write_group_sets(a, d, prm, h.names);
        phase("group sets");
    }
    // --marker-coverage: one more pass over the same reads, placed like --group-sets (first replica, whole file, after
    // everything else the run prints and writes).
    // --marker-track rides on the same pass: one stream of the reads fills the handle that both files are folded from.
    if (!a.out_file_marker_coverage.empty() || !a.out_file_marker_track.empty()) {
        MarkerTrackRows track;
        const bool want_track = !a.out_file_marker_track.empty();
        write_marker_coverage(a, idx, d, prm, h.names, want_track ? &track : nullptr);
        if (!a.out_file_marker_coverage.empty()) phase("marker coverage");
        if (want_track) {
            write_marker_track(a, idx, track, h.names);
            phase("marker track");
        }
    }
    // --bootstrap / --bootstrap-em: one more pass over the same reads, placed like --group-sets; mode, pairing, k,
    // cutoff and the fixed accuracy are the run's own. --bootstrap's intervals bound the initial percentages (the first
    // vector printed above), --bootstrap-em's the EM-refined ones: the pass then fills one histogram per replicate
    // through the run's finalized histogram, which is kept until here for it.
    if (!a.out_file_bootstrap.empty() || !a.out_file_bootstrap_em.empty()) {
        write_bootstrap(a, d, prm, h.names, u_ref, tot_ref, em, h.counts, percent);
        phase("bootstrap");
    }
    // --dedup: two more passes over the same reads, placed like --group-sets: the percentages with every distinct read
    // (pair) counted once, beside the run's own.
    if (!a.out_file_dedup.empty()) {
        write_dedup(a, idx, d, prm, h.names, u_ref, tot_ref, h.counts, initial, percent);
        phase("dedup");
    }
    speq_em_free(em);
    // The device replica, its pinned pipeline slots and the index are left to process exit: unpinning and freeing
    // them explicitly costs ~0.07 s and the process ends right after this.
    (void)d;
    (void)idx;
    phase("output");
    phase.since_launch("launch -> done");
    return 1;  // the reference's scan returns 1 (fm_scanner.cpp:280); main ignores it
}

}  // namespace

int main(int argc, char** argv) {
    CmdArguments a;
    try {
        a = speq::args::parse(argc, argv);
    } catch (const speq::args::ParseError& e) {
        std::string sub = argc > 1 ? argv[1] : "";
        if (sub == "index" || sub == "scan" || sub == "all")
            std::cerr << "speq " << sub << " | argument parsing error:  " << e.what() << "\n";
        else
            std::cerr << "SPeQ Error: " << e.what() << "\n";
        return 1;
    }
    if (!a.is_parsed) return 0;
    try {
        // one process per GPU: rank 0 alone builds the index; the others wait for it at the rendezvous in run_scan
        const Dist dd = a.is_scanner ? dist_from_env(a) : Dist{};
        dist_clear_stale(dd);
        const bool other_rank = dd.rank != 0;
        if (a.is_indexer && !other_rank) run_index(a);
        if (a.is_scanner) {
            run_scan(a);
            // Everything is written and the GPU idle: leave without the runtime's teardown (unpinning the stream's
            // slots, freeing the replica: ~0.2 s of a config-3 scan, profiles/r06/cli_trace_*), which process exit
            // does in the kernel anyway. SPEQ_FULL_EXIT=1 keeps the ordinary exit.
            const char* fe = std::getenv("SPEQ_FULL_EXIT");
            if (!(fe && fe[0] == '1')) {
                std::cout.flush();
                std::cerr.flush();
                std::fflush(nullptr);
                std::_Exit(0);
            }
        }
    } catch (const std::exception& e) {
        std::cerr << "speq: error: " << e.what() << "\n";
        return 2;
    }
    return 0;
}
