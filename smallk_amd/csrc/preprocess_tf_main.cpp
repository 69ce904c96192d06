// smallk_amd/csrc/preprocess_tf_main.cpp -- the `preprocess_tf` command line tool on the MI355X.
// Same flags, defaults, messages, files and flow as the reference tool (preprocessor/src/command_line.cpp:26-164,
// preprocessor/src/main.cpp:37-282): read matrix.mtx, dictionary.txt and documents.txt from --indir, prune and score on the
// device (smk_preprocess), write reduced_matrix.mtx, reduced_dictionary.txt and reduced_documents.txt to --outdir.
// Arguments and input files are checked before the device is touched.
#include <chrono>
#include <cstdlib>
#include <limits>
#include <stdexcept>

#include "cli_common.h"

namespace {

struct Options {
    std::string indir, outdir;
    int terms_per_doc = 5, docs_per_term = 3, max_iter = 1000, precision = 4, boolean_mode = 0;
};

void PrintUsage(const std::string& prog)
{
    std::cout << std::endl;
    std::cout << "Usage: " << prog << std::endl;
    std::cout << "          --indir  <path> " << std::endl;
    std::cout << "        [--outdir  (defaults to current directory)] " << std::endl;
    std::cout << "        [--docs_per_term  3] " << std::endl;
    std::cout << "        [--terms_per_doc  5] " << std::endl;
    std::cout << "        [--maxiter  1000] " << std::endl;
    std::cout << "        [--precision  4] " << std::endl;
    std::cout << "        [--boolean_mode  0] " << std::endl;
    std::cout << std::endl;
}

void PrintOpts(const Options& o)
{
    std::cout << "\n      Command line options: \n" << std::endl;
    std::cout << "\t             indir: " << o.indir << std::endl;
    std::cout << "\t            outdir: " << o.outdir << std::endl;
    std::cout << "\t     docs_per_term: " << o.docs_per_term << std::endl;
    std::cout << "\t     terms_per_doc: " << o.terms_per_doc << std::endl;
    std::cout << "\t          max_iter: " << o.max_iter << std::endl;
    std::cout << "\t         precision: " << o.precision << std::endl;
    std::cout << "\t      boolean_mode: " << o.boolean_mode << std::endl;
    std::cout << std::endl;
}

// an invalid numeric value: the reference throws std::runtime_error here (utils.cpp InvalidValue) and lets it end the process;
// main() below prints the same message and returns -1, as the other tools of this project do
[[noreturn]] void InvalidValue(const std::string& arg)
{
    throw std::runtime_error("Invalid value specified for command-line argument " + arg);
}

// flags are told apart by their first letter after "--", values follow them (command_line.cpp:56-125)
void ParseCommandLine(int argc, char* argv[], Options& o)
{
    for (int k = 1; k + 1 < argc; k += 2) {
        const char* a = argv[k];
        if (a[0] != '-' || a[1] != '-') continue;
        const int v = atoi(argv[k + 1]);
        switch (a[2]) {
        case 'm': if (v <= 0) InvalidValue(a); o.max_iter = v; break;
        case 'p':
            if (v <= 0) InvalidValue(a);
            o.precision = std::min(v, std::numeric_limits<double>::max_digits10);
            break;
        case 'i': o.indir = argv[k + 1]; break;
        case 'o': o.outdir = argv[k + 1]; break;
        case 'd': if (v <= 0) InvalidValue(a); o.docs_per_term = v; break;
        case 't': if (v <= 0) InvalidValue(a); o.terms_per_doc = v; break;
        case 'b': if (v < 0) InvalidValue(a); o.boolean_mode = v == 0 ? 0 : 1; break;
        default: break;
        }
    }
}

bool IsValid(const Options& o)
{
    if (o.indir.empty()) {
        std::cerr << "preprocessor error: required command line argument --indir not found" << std::endl;
        return false;
    }
    if (o.max_iter <= 0) {
        std::cerr << "preprocessor error: iteration count must be a positive integer" << std::endl;
        return false;
    }
    if (o.docs_per_term <= 0) {
        std::cerr << "preprocessor error: docs_per_term must be a positive integer" << std::endl;
        return false;
    }
    if (o.terms_per_doc <= 0) {
        std::cerr << "preprocessor error: terms_per_doc must be a positive integer" << std::endl;
        return false;
    }
    return true;
}

// WriteStringsToFile (main.cpp:255-282)
bool WriteStrings(const std::string& path, const std::vector<std::string>& strings, const std::vector<unsigned>& idx, unsigned n)
{
    std::ofstream out(path);
    if (!out) return false;
    std::string buf;
    for (unsigned s = 0; s < n; ++s) {
        buf += strings[idx[s]];
        buf += '\n';
    }
    out << buf;
    return (bool)out;
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char* argv[])
{
    const std::string prog(argv[0]);
    if (argc == 1) {
        PrintUsage(prog);
        return 0;
    }
    Options o;
    try {
        ParseCommandLine(argc, argv, o);
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return -1;
    }
    if (!IsValid(o)) return -1;
    if (!cli::directory_exists(o.indir)) {
        std::cerr << "\npreprocessor: the specified input directory " << o.indir << " does not exist." << std::endl;
        return -1;
    }
    if (!o.outdir.empty() && !cli::directory_exists(o.outdir)) {
        std::cerr << "\npreprocessor: the specified output directory " << o.outdir << " does not exist." << std::endl;
        return -1;
    }
    const std::string inputdir = cli::ensure_trailing_sep(o.indir);
    const std::string infile = inputdir + "matrix.mtx", indict = inputdir + "dictionary.txt", indocs = inputdir + "documents.txt";
    const std::string outputdir = o.outdir.empty() ? std::string() : cli::ensure_trailing_sep(o.outdir);
    const std::string outfile = outputdir + "reduced_matrix.mtx", outdict = outputdir + "reduced_dictionary.txt",
                      outdocs = outputdir + "reduced_documents.txt";

    std::vector<std::string> dictionary, documents;
    if (!cli::load_strings(indict, dictionary)) {
        std::cerr << "\npreprocessor: could not open dictionary file " << indict << std::endl;
        return -1;
    }
    const unsigned num_terms = (unsigned)dictionary.size();
    if (!cli::load_strings(indocs, documents)) {
        std::cerr << "\npreprocessor: could not open documents file " << indocs << std::endl;
        return -1;
    }
    const unsigned num_docs = (unsigned)documents.size();

    o.indir = inputdir;
    o.outdir = outputdir.empty() ? std::string("current directory") : outputdir;
    PrintOpts(o);

    std::cout << "Loading input matrix " << infile << std::endl;
    auto t = std::chrono::steady_clock::now();
    unsigned height = 0, width = 0, nnz = 0;
    std::vector<unsigned> cols, rows;
    std::vector<double> data;
    bool loaded = smk_load_matrix_market(infile.c_str(), &height, &width, &nnz, nullptr, nullptr, nullptr) == 1;
    if (loaded) {
        cols.resize((size_t)width + 1);
        rows.resize(nnz ? nnz : 1);
        data.resize(nnz ? nnz : 1);
        loaded = smk_load_matrix_market(infile.c_str(), &height, &width, &nnz, cols.data(), rows.data(), data.data()) == 1;
    }
    if (!loaded) {
        std::cerr << "\npreprocessor: could not load file " << infile << std::endl;
        return -1;
    }
    std::cout << "\tInput file load time: " << seconds_since(t) << "s." << std::endl;

    if (num_terms < height) {
        std::cerr << "\npreprocessor error: expected " << height << " terms in the dictionary; found " << num_terms << "." << std::endl;
        return -1;
    }
    if (num_docs < width) {
        std::cerr << "\npreprocessor error: expected " << width << " strings in the documents file; found " << num_docs << "." << std::endl;
        return -1;
    }

    // the device from here on
    t = std::chrono::steady_clock::now();
    if (smk_initialize(-1) != SMK_OK) {
        std::cerr << "\npreprocessor: " << smk_last_error() << std::endl;
        return -1;
    }
    smk_preprocess_options po;
    po.max_iter = (unsigned)o.max_iter;
    po.docs_per_term = (unsigned)o.docs_per_term;
    po.terms_per_doc = (unsigned)o.terms_per_doc;
    po.boolean_mode = o.boolean_mode;
    smk_preprocess_result* res = nullptr;
    std::cout << "\nStarting iterations..." << std::endl;
    const int rc = smk_preprocess(&po, height, width, nnz, cols.data(), rows.data(), data.data(), &res);
    if (rc != SMK_OK && rc != SMK_FAILURE) {
        std::cerr << "\npreprocessor: " << smk_last_error() << std::endl;
        return -1;
    }
    unsigned h = 0, w = 0, n = 0, iters = 0;
    smk_preprocess_result_sizes(res, &h, &w, &n, &iters);
    std::vector<unsigned> log((size_t)iters * 3);
    smk_preprocess_result_log(res, log.data());
    for (unsigned i = 0; i < iters; ++i)
        std::cout << "\t[" << (i + 1) << "] height: " << log[3 * i] << ", width: " << log[3 * i + 1] << ", nonzeros: " << log[3 * i + 2]
                  << std::endl;
    if (rc == SMK_FAILURE) {
        std::cerr << "Preprocessor: all columns were pruned." << std::endl;
    } else {
        std::cout << "Iterations finished." << std::endl;
        std::cout << "\tNew height: " << h << std::endl;
        std::cout << "\tNew width: " << w << std::endl;
        std::cout << "\tNew nonzero count: " << n << std::endl;
    }
    std::cout << "Processing time: " << seconds_since(t) << "s." << std::endl;
    std::cout << std::endl;
    if (rc == SMK_FAILURE) {
        std::cerr << "\npreprocessor: matrix has dimension zero." << std::endl;
        std::cerr << "no output files will be written" << std::endl;
        smk_preprocess_result_destroy(res);
        return 0;           // main.cpp:194-195 returns `false`
    }

    std::cout << "Writing output matrix '" << outfile << "'" << std::endl;
    t = std::chrono::steady_clock::now();
    if (smk_preprocess_write_mtx(res, outfile.c_str(), (unsigned)o.precision) != SMK_OK) {
        std::cerr << "\npreprocessor: could not write file " << outfile << std::endl;
        smk_preprocess_result_destroy(res);
        return -1;
    }
    std::cout << "Output file write time: " << seconds_since(t) << "s." << std::endl;

    std::vector<unsigned> term_indices(h), doc_indices(w);
    if (smk_preprocess_result_download(res, term_indices.data(), doc_indices.data(), nullptr, nullptr, nullptr) != SMK_OK) {
        std::cerr << "\npreprocessor: " << smk_last_error() << std::endl;
        smk_preprocess_result_destroy(res);
        return -1;
    }
    smk_preprocess_result_destroy(res);
    std::cout << "Writing dictionary file '" << outdict << "'" << std::endl;
    t = std::chrono::steady_clock::now();
    if (!WriteStrings(outdict, dictionary, term_indices, h)) std::cerr << "\npreprocessor: could not write file " << outdict << std::endl;
    double elapsed = seconds_since(t);
    std::cout << "Writing documents file '" << outdocs << "'" << std::endl;
    t = std::chrono::steady_clock::now();
    if (!WriteStrings(outdocs, documents, doc_indices, w)) std::cerr << "\npreprocessor: could not write file " << outdocs << std::endl;
    elapsed += seconds_since(t);
    std::cout << "Dictionary + documents write time: " << elapsed << "s." << std::endl;
    return 0;
}
