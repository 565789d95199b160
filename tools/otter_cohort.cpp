// otter_cohort — sample BAMs to one joint VCF on MI355X through the C-ABI alone (include/otter_gpu.h): `otter assemble` per sample and
// `otter genotype` over their alleles in one pass (otg_cohort_files), the alleles never leaving the device in between.  Host C++ only.
//   otter_cohort -b regions.bed -r ref.fa [the assemble options of otter_assemble: --haps -p -l -o L[,R] -a N -m Q -q RQ -c COV -F f -A len,f -e err
//                -h bw[,len,bw] -f flank -s sim -t threads --batch N --gpus 0,1,.. --wfa-heuristic ..] [-E gt-max-error] [-S gt-max-cosdis]
//                [--gt-metric length|edit] [--alleles-prefix P [--alleles-bam]] [--matrix FILE [-k K]] NAME=reads.bam ...
// The VCF goes to stdout.  NAME is the sample's `-R` and its VCF column.  --alleles-prefix P also writes the allele records of every sample, as
// `otter assemble -R NAME` prints them, to P<NAME>.sam; with --alleles-bam to P<NAME>.bam + P<NAME>.bam.bai instead (otg_bam_sink).
// --gt-metric edit clusters the alleles by exact edit distance instead of the length ratio (OTG_GT_METRIC_EDIT); length is the default.
// --matrix FILE also writes the k-mer usage matrix of the joint alleles, what `otter vcf2mat -k K` prints for the VCF (K defaults to 3).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../include/otter_gpu.h"

static int write_stdout(void*, const char* data, uint64_t len) { return fwrite(data, 1, (size_t)len, stdout) == (size_t)len ? 0 : 1; }
static int write_file(void* user, const char* data, uint64_t len) { return fwrite(data, 1, (size_t)len, (FILE*)user) == (size_t)len ? 0 : 1; }
static int write_sample(void* user, uint32_t sample, const char* data, uint64_t len)
{
  FILE* f = (*(std::vector<FILE*>*)user)[sample];
  return fwrite(data, 1, (size_t)len, f) == (size_t)len ? 0 : 1;
}

static int write_sample_bam(void* user, uint32_t sample, const char* data, uint64_t len)
{
  return otg_bam_sink_write((*(std::vector<otg_bam_sink*>*)user)[sample], data, len);
}

static std::vector<std::string> split(const std::string& s, char c)
{
  std::vector<std::string> out; size_t a = 0;
  for (;;) { const size_t b = s.find(c, a); out.push_back(s.substr(a, b == std::string::npos ? b : b - a)); if (b == std::string::npos) break; a = b + 1; }
  return out;
}

static const char* USAGE = "usage: otter_cohort -b <BED> -r <FASTA> [options] NAME=<BAM> [NAME=<BAM> ...]   ('--bed', '--reference' and at least one sample are required)\n";

int main(int argc, char** argv)
{
  otg_cohort_job job; memset(&job, 0, sizeof job);
  otg_params_default(&job.params);
  job.ingest.offset_l = 1; job.ingest.offset_r = 0; job.ingest.threads = 1;       // --offset 1,0 and -t 1: the reference's defaults
  std::string bed, ref, prefix, matrix;
  job.matrix_k = 3;                                                               // -k of `otter vcf2mat`
  std::vector<std::string> names, bams;
  std::vector<int32_t> devs;
  bool alleles_bam = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto val = [&]() -> std::string { if (i + 1 >= argc) { fprintf(stderr, "[ERROR] %s needs a value\n", a.c_str()); exit(1); } return argv[++i]; };
    if (a == "-b" || a == "--bed") bed = val();
    else if (a == "-r" || a == "--reference") ref = val();
    else if (a == "-E" || a == "--gt-max-error") job.params.gt_max_error = atof(val().c_str());
    else if (a == "-S" || a == "--gt-max-cosdis") job.params.gt_max_cosdis = atof(val().c_str());
    else if (a == "--gt-metric") {
      const std::string m = val();
      if (m == "length") job.gt_metric = OTG_GT_METRIC_LENGTH;
      else if (m == "edit") job.gt_metric = OTG_GT_METRIC_EDIT;
      else { fprintf(stderr, "[ERROR] --gt-metric length | edit\n"); return 1; }
    }
    else if (a == "--alleles-prefix") prefix = val();
    else if (a == "--alleles-bam") alleles_bam = true;
    else if (a == "--matrix") matrix = val();
    else if (a == "-k" || a == "--kmer-size") job.matrix_k = atoi(val().c_str());
    else if (a == "--haps") job.params.ignore_haps = 0;
    else if (a == "-p" || a == "--non-primary") job.ingest.nonprimary = 1;
    else if (a == "-l" || a == "--omit-nonspanning") job.ingest.omit_nonspanning = 1;
    else if (a == "-o" || a == "--offset") { auto v = split(val(), ','); job.ingest.offset_l = atoi(v[0].c_str()); job.ingest.offset_r = v.size() > 1 ? atoi(v[1].c_str()) : job.ingest.offset_l; }
    else if (a == "-a" || a == "--max-alleles") job.params.max_alleles = atoi(val().c_str());
    else if (a == "-m" || a == "--mapq") job.ingest.mapq = atoi(val().c_str());
    else if (a == "-q" || a == "--read-quality") job.ingest.read_quality = atof(val().c_str());
    else if (a == "-c" || a == "--max-cov") job.params.max_cov = atoi(val().c_str());
    else if (a == "-F" || a == "--cov-fraction") job.params.min_cov_fraction = atof(val().c_str());
    else if (a == "-A" || a == "--cov-fraction-large") { auto v = split(val(), ','); if (v.size() == 2) { job.params.min_cov_fraction2_l = atoi(v[0].c_str()); job.params.min_cov_fraction2_f = atof(v[1].c_str()); } }
    else if (a == "-e" || a == "--max-error") job.params.max_error = atof(val().c_str());
    else if (a == "-h" || a == "--bandwidth") { auto v = split(val(), ','); job.params.bandwidth_short = atof(v[0].c_str());
      if (v.size() == 3) { job.params.bandwidth_length = atoi(v[1].c_str()); job.params.bandwidth_long = atof(v[2].c_str()); } else job.params.bandwidth_long = job.params.bandwidth_short; }
    else if (a == "-f" || a == "--flank-size") job.params.flank = atoi(val().c_str());
    else if (a == "-s" || a == "--min-sim") job.params.min_sim = atof(val().c_str());
    else if (a == "-t" || a == "--threads") job.ingest.threads = atoi(val().c_str());
    else if (a == "--batch") job.batch_regions = (uint32_t)atoi(val().c_str());
    else if (a == "--gpus") { for (auto& d : split(val(), ',')) devs.push_back(atoi(d.c_str())); }
    else if (a == "--wfa-heuristic") {
      const std::string h = val();
      if (h == "none") job.params.heuristic = OTG_HEURISTIC_NONE;
      else if (h.rfind("wfadaptive", 0) == 0) {
        job.params.heuristic = OTG_HEURISTIC_WFADAPTIVE;
        if (h.size() > 10 && h[10] == ':') { auto v = split(h.substr(11), ','); if (v.size() != 3) { fprintf(stderr, "[ERROR] --wfa-heuristic wfadaptive:<min_wavefront_length>,<max_distance_threshold>,<steps>\n"); return 1; }
          job.params.heur_min_wavefront_length = atoi(v[0].c_str()); job.params.heur_max_distance_threshold = atoi(v[1].c_str()); job.params.heur_steps_between_cutoffs = atoi(v[2].c_str()); }
      } else { fprintf(stderr, "[ERROR] --wfa-heuristic none | wfadaptive[:a,b,c]\n"); return 1; }
    }
    else if (a.size() && a[0] == '-') { fprintf(stderr, "[ERROR] unknown option %s\n", a.c_str()); return 1; }
    else {
      const size_t eq = a.find('=');
      if (eq == std::string::npos) { fprintf(stderr, "[ERROR] sample '%s' is not NAME=<BAM>\n", a.c_str()); return 1; }
      names.push_back(a.substr(0, eq)); bams.push_back(a.substr(eq + 1));
    }
  }
  if (bams.empty() || bed.empty() || ref.empty()) { fputs(USAGE, stderr); return 1; }
  std::vector<const char*> pn, pb;
  for (size_t s = 0; s < bams.size(); ++s) { pn.push_back(names[s].c_str()); pb.push_back(bams[s].c_str()); }
  job.n_samples = (uint32_t)bams.size(); job.bam_paths = pb.data(); job.sample_names = pn.data();
  job.bed_path = bed.c_str(); job.fasta_path = ref.c_str();
  job.n_devices = (int32_t)devs.size(); job.devices = devs.empty() ? nullptr : devs.data();
  if (alleles_bam && prefix.empty()) { fprintf(stderr, "usage: --alleles-bam needs --alleles-prefix\n"); return 1; }
  std::vector<FILE*> files;
  std::vector<otg_bam_sink*> sinks;
  if (alleles_bam) {
    otg_bam_sink_opts so; memset(&so, 0, sizeof so);
    so.threads = job.ingest.threads; so.level = -1;
    for (size_t s = 0; s < bams.size(); ++s) {
      otg_bam_sink* k = nullptr;
      if (otg_bam_sink_open((prefix + names[s] + ".bam").c_str(), &so, &k) != OTG_OK) {
        fprintf(stderr, "[ERROR] %s\n", otg_last_error(nullptr));
        for (otg_bam_sink* x : sinks) otg_bam_sink_abort(x);
        return 1;
      }
      sinks.push_back(k);
    }
    job.allele_write = write_sample_bam; job.allele_user = &sinks;
  } else if (!prefix.empty()) {
    for (size_t s = 0; s < bams.size(); ++s) {
      const std::string path = prefix + names[s] + ".sam";
      FILE* f = fopen(path.c_str(), "wb");
      if (!f) { fprintf(stderr, "[ERROR] cannot write %s\n", path.c_str()); return 1; }
      files.push_back(f);
    }
    job.allele_write = write_sample; job.allele_user = &files;
  }
  FILE* fmat = nullptr;
  if (!matrix.empty()) {
    fmat = fopen(matrix.c_str(), "wb");
    if (!fmat) { fprintf(stderr, "[ERROR] cannot write %s\n", matrix.c_str()); for (otg_bam_sink* x : sinks) otg_bam_sink_abort(x); return 1; }
    job.matrix_write = write_file; job.matrix_user = fmat;
  }
  otg_job_stats st;
  int rc = otg_cohort_files(&job, write_stdout, nullptr, &st);
  fflush(stdout);
  const bool matrix_lost = fmat && fclose(fmat) != 0;
  for (FILE* f : files) fclose(f);
  if (rc != OTG_OK) {
    const std::string job_err = otg_last_error(nullptr);
    std::string why;
    for (otg_bam_sink* x : sinks) { if (why.empty()) why = otg_bam_sink_error(x); otg_bam_sink_abort(x); }
    fprintf(stderr, "[ERROR] otter_cohort failed (%d): %s%s%s\n", rc, job_err.c_str(), why.empty() ? "" : ": ", why.c_str());
    return 1;
  }
  for (size_t s = 0; s < sinks.size(); ++s) {
    if (rc == OTG_OK) rc = otg_bam_sink_close(sinks[s], nullptr); else otg_bam_sink_abort(sinks[s]);
  }
  if (rc != OTG_OK) { fprintf(stderr, "[ERROR] otter_cohort failed (%d): %s\n", rc, otg_last_error(nullptr)); return 1; }
  if (matrix_lost) { fprintf(stderr, "[ERROR] cannot write %s\n", matrix.c_str()); return 1; }
  fprintf(stderr, "otter_cohort: %u samples, %llu regions (%llu with a VCF line), %llu reads, %llu alleles, %.1f MB out; %.3f s wall on %u GPU(s); stage busy ms: ingest %.0f, hot path %.0f, emit %.0f\n",
          job.n_samples, (unsigned long long)st.n_regions, (unsigned long long)st.n_regions_ok, (unsigned long long)st.n_reads, (unsigned long long)st.n_alleles, st.output_bytes / 1e6,
          st.ms_total / 1e3, st.n_devices, st.ms_ingest, st.ms_hot_path, st.ms_emit);
  return 0;
}
