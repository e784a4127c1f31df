"""The artifact-model stage of `filter_variants` on the MI355X engine (reference tools/filter_variants.py:292-320, :350-357:
`generate_posterior_data` + `MemoryMappedData.from_generator`): every candidate of a dataset tar goes through the model's forward and
comes out as a read-less Datum row whose info array is its embedding and whose CACHED_ARTIFACT_LOGIT is its logit -- the input of
the posterior model.  The tool reads a dataset tar in the reference's format (or, with --test_dataset, Mutect2's plain text) and writes
the posterior data as a tar in the same format; the stages behind it are switched on by their flags, below.

    python -m permutect_amd.tools.filter_variants --test_dataset_tar candidates.tar --artifact_model model.pt --output posterior.tar

With `--input VCF --contigs_table T [--maf_segments F] [--normal_maf_segments F]` the candidates are annotated first (reference
data/memory_mapped_data.py:131-175 behind `make_posterior_data_loader`; data/site_annotation.py here): a freshly preprocessed tar
carries NaN in ALLELE_FREQUENCY, MAF and NORMAL_MAF; the allele frequency comes from the VCF's POPAF, the two minor-allele fractions
from the segment files (0.5 outside every segment), and candidates that the VCF does not hold or that Mutect2 filtered as
`contamination` or `slippage` are dropped -- one launch over the candidates' identity columns (pmt_annotate_sites).  Every rank reads
the same files and gets the same kept list: no collective.  Without `--input` the three columns are taken as the tar has them.

With `--genomic_span` the posterior stage follows (reference tools/filter_variants.py:244-289; architecture/posterior_model.py): rank 0
turns the posterior data into device-resident columns, learns the priors and allele-fraction spectra
(`PosteriorModel.learn_priors_and_spectra`), sets the error-probability threshold of every variant type and writes per-candidate
probabilities, calls and the thresholds as arrays to `--calls_output` (.npz).  Context-dependent SNV priors stay off in every epoch
unless `--context_dependent_snv_priors` is given: then the reference's regime runs (context on for the second half of the epochs, the
5 x 5 x 5 x 5 table `priors.somatic_snv_log_priors_rrra` refitted after each of them and used for the thresholds and calls; it is part of
the state_dict in the .npz).  The table's fit is a deterministic estimator of the reference's generative model of per-context mutation
rates, one persistent launch on the device -- NOT the reference's stochastic pymc ADVI fit, whose numbers it does not claim to match
(architecture/posterior_priors.py).  The artifact priors and spectra stored in the model file are loaded and, as in the reference
(tools/filter_variants.py:242, :265), not used.

    ... --genomic_span 3e9 --calls_output calls.npz [--num_spectrum_iterations 10] [--germline_mode | --no_germline_mode] [--het_beta B]
        [--context_dependent_snv_priors] [--evaluation_output eval.npz]

With `--evaluation_output` and candidates that carry truth labels (reference tools/filter_variants.py:381-411, :534-617) rank 0 then scores
the calls it has just written: one pass over the rows on the device (architecture/posterior_evaluation.py: pmt_posterior_evaluate)
tallies the error logit by label, the cached artifact logit by most-confident call, the filter's confusion counts and the mistakes into
integer tables; the .npz holds the tables, the sensitivity / precision curve of every variant type over all counts
(metrics/accuracy_curves.py), the thresholds as logits, sensitivity and precision at those thresholds, and the row indices and bad calls
of the mistakes.  The filter decisions are the `filtered_b` of --calls_output, passed on.  The reference's plots are not drawn.

With `--output_vcf PATH` (needs --input, --contigs_table and --genomic_span; reference tools/filter_variants.py:369-617
`apply_filtering_to_vcf`) rank 0 then writes the filtered VCF (tools/filtered_vcf.py; csrc/pmt_vcf.hip): every record of --input finds
its candidate on the device, gets its FILTER text (the trusted Mutect2 filters it had, the error call's name when its candidate is
filtered, `seq_error` when it has no candidate and no alt depth) and, with a candidate, POST, PRIOR, SPECLL, ARTLOD and NORMLL formatted
as Python's `{:.3f}`; every other byte is the input's.  The VCF is read once per run: the site annotation and the writer share the pass
(data/vcf_text.py).  The decisions are again the `filtered_b` of --calls_output.  Plain text, or gzip when PATH ends in `.gz`.

    ... --input in.vcf --contigs_table contigs.table --genomic_span 3e9 --calls_output calls.npz --output_vcf filtered.vcf

Under torchrun (`python -m torch.distributed.run --nproc-per-node N -m permutect_amd.tools.filter_variants ...`: WORLD_SIZE > 1) the
candidates are cut into N contiguous shards, one process per GPU, no collective on the data path; rank 0 concatenates the shards'
rows in dataset order and writes the tar (tools/posterior_data.py: make_posterior_mmap)."""
from __future__ import annotations

import argparse
import time

import torch

from permutect_amd import constants
from permutect_amd.architecture.artifact_model import load_model
from permutect_amd.data.memory_mapped_data import MemoryMappedData
from permutect_amd.data.reads_dataset import ReadsDataset
from permutect_amd.tools.posterior_data import make_posterior_mmap
from permutect_amd.training.distributed import init_from_env

TEST_DATASET_TAR_NAME = "test_dataset_tar"
TEST_DATASET_NAME = "test_dataset"      # (reference constants.py: TEST_DATASET_NAME)
ARTIFACT_MODEL_NAME = "artifact_model"  # (reference constants.py: ARTIFACT_MODEL_NAME)
GENOMIC_SPAN_NAME = "genomic_span"       # (reference constants.py: GENOMIC_SPAN_NAME)
CONTIGS_TABLE_NAME = "contigs_table"             # (reference constants.py: CONTIGS_TABLE_NAME)
MAF_SEGMENTS_NAME = "maf_segments"               # (reference constants.py: MAF_SEGMENTS_NAME)
NORMAL_MAF_SEGMENTS_NAME = "normal_maf_segments"  # (reference constants.py: NORMAL_MAF_SEGMENTS_NAME)
POSTERIOR_BATCH_SIZE = 64               # the reference's loader for the posterior model takes its --batch_size, 64 by default
DEFAULT_BATCH_SIZE = 65536  # the reference's flag defaults to 64 (tools/filter_variants.py:81); the rows do not depend on it


def main_without_parsing(args, log=print):
    if torch.cuda.device_count() == 0:
        raise RuntimeError("permutect_amd filters on an MI355X (ROCm device 'cuda'); there is no CPU path")
    dist, rank, world, device = init_from_env()  # this rank's card and the process group, before anything else touches the GPU
    model, _, _ = load_model(getattr(args, ARTIFACT_MODEL_NAME), device=device)
    data = load_candidates(args, device)
    vcf = None
    if getattr(args, constants.INPUT_NAME, None) is not None:
        vcf = read_input_vcf(args)
        data = annotate_candidates(args, data, device, log if rank == 0 else (lambda *a, **k: None), vcf=vcf)
    dataset = ReadsDataset(data)
    t0 = time.perf_counter()
    posterior = make_posterior_mmap(dataset, model, getattr(args, constants.BATCH_SIZE_NAME), device=device,
                                    chunk_variants=getattr(args, "chunk_variants", None), rank=rank, world_size=world)
    if rank == 0:
        dt = time.perf_counter() - t0
        log(f"{len(posterior)} candidates through the artifact model on {world} GPU(s) in {dt:.3f} s ({len(posterior) / max(dt, 1e-9) / 1e6:.2f} M/s, "
            "disk to posterior rows)")
        posterior.save_to_tarfile(getattr(args, constants.OUTPUT_NAME))
        if posterior_stage_requested(args):  # (sequential: under torchrun the other ranks wait at the barrier below)
            run_posterior_stage(args, posterior, device, log, vcf=vcf)
    if dist is not None:
        dist.barrier()
    return posterior


def load_candidates(args, device) -> MemoryMappedData:
    """--test_dataset_tar, or --test_dataset: the text preprocessed in memory (data/plain_text_data.py)"""
    tar, text = getattr(args, TEST_DATASET_TAR_NAME, None), getattr(args, TEST_DATASET_NAME, None)
    if (tar is None) == (text is None):
        raise ValueError(f"exactly one of --{TEST_DATASET_TAR_NAME} and --{TEST_DATASET_NAME} is required")
    if tar is not None:
        return MemoryMappedData.load_from_tarfile(tar)
    from permutect_amd.data.plain_text_data import make_normalized_mmap_data
    return make_normalized_mmap_data([text], device=device)


def read_input_vcf(args):
    """--input read ONCE (data/vcf_text.py): the site table of the annotation and, for --output_vcf, the header and the record table"""
    from permutect_amd.data import site_annotation as S
    from permutect_amd.data.vcf_text import read_vcf
    contigs_path = getattr(args, CONTIGS_TABLE_NAME, None)
    if contigs_path is None:
        raise ValueError(f"--{constants.INPUT_NAME} names candidates by contig name: it needs --{CONTIGS_TABLE_NAME}")
    return read_vcf(getattr(args, constants.INPUT_NAME), S.read_contig_indices(contigs_path))


def annotate_candidates(args, data: MemoryMappedData, device, log=print, vcf=None) -> MemoryMappedData:
    """--input: the three annotated float columns from the VCF and the segment files, the candidates outside the VCF or with a trusted
    Mutect2 filter dropped (data/site_annotation.py).  `vcf`: the input VCF as `read_input_vcf` has read it (else it is read here)."""
    from permutect_amd.data import site_annotation as S
    contigs_path = getattr(args, CONTIGS_TABLE_NAME, None)
    if contigs_path is None:
        raise ValueError(f"--{constants.INPUT_NAME} names candidates by contig name: it needs --{CONTIGS_TABLE_NAME}")
    t0 = time.perf_counter()
    contigs = S.read_contig_indices(contigs_path)
    sites = vcf.sites if vcf is not None else S.read_vcf_sites(getattr(args, constants.INPUT_NAME), contigs)
    segments = S.read_segments(getattr(args, MAF_SEGMENTS_NAME, None), contigs)
    normal_segments = S.read_segments(getattr(args, NORMAL_MAF_SEGMENTS_NAME, None), contigs)
    t1 = time.perf_counter()
    annotated, counts = S.annotate_dataset(data, sites, segments, normal_segments, device)
    t2 = time.perf_counter()
    log(f"site annotation: {len(data)} candidates against {len(sites)} sites ({sites.num_records} VCF records), {len(segments)} / "
        f"{len(normal_segments)} segments: " + ", ".join(f"{name} {count}" for name, count in counts.items())
        + f"; read {t1 - t0:.3f} s, annotate {t2 - t1:.3f} s")
    return annotated


def posterior_stage_requested(args) -> bool:
    return getattr(args, GENOMIC_SPAN_NAME, None) is not None


def posterior_outputs(model, rows, thresholds, losses, germline_mode: bool) -> dict:
    """the arrays of `--calls_output`: per candidate the four ingredient tensors' first three, the posterior probabilities, the error
    probability, whether it is filtered (reference `apply_filtering_to_vcf`, :535-537: error probability strictly above its variant
    type's threshold) and the most probable call; the thresholds by variant type; the per-epoch losses; the model's state_dict"""
    from permutect_amd.enums import Call, Variation
    with torch.no_grad():
        log_priors_bc, spectra_log_lks_bc, normal_log_lks_bc, log_posteriors_bc = model.log_posterior_and_ingredients(rows)
        probs_bc = torch.nn.functional.softmax(log_posteriors_bc, dim=1)
        error_probs_b = 1 - probs_bc[:, Call.GERMLINE if germline_mode else Call.SOMATIC]
        thresholds_v = torch.tensor([thresholds[v] for v in Variation], dtype=error_probs_b.dtype, device=error_probs_b.device)
        filtered_b = error_probs_b > thresholds_v[rows.variant_types.long()]
        most_confident_call_b = torch.max(probs_bc, dim=-1).indices
    out = {"posterior_probabilities_bc": probs_bc, "error_probabilities_b": error_probs_b, "log_priors_bc": log_priors_bc,
           "spectra_log_lks_bc": spectra_log_lks_bc, "normal_log_lks_bc": normal_log_lks_bc, "thresholds_v": thresholds_v,
           "filtered_b": filtered_b, "most_confident_call_b": most_confident_call_b, "losses": torch.tensor(losses, dtype=torch.float64)}
    out.update(model.state_dict())
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def run_posterior_stage(args, posterior: MemoryMappedData, device, log=print, vcf=None):
    import numpy as np
    from permutect_amd.architecture.posterior_model import PosteriorModel, PosteriorRows
    germline_mode, no_germline_mode = getattr(args, "germline_mode", False), getattr(args, "no_germline_mode", False)
    if germline_mode and no_germline_mode:
        raise ValueError("--germline_mode and --no_germline_mode are incompatible")
    t0 = time.perf_counter()
    rows = PosteriorRows.from_data(posterior, device=device)
    n = len(rows)
    model = PosteriorModel(getattr(args, "initial_log_variant_prior"), getattr(args, "initial_log_artifact_prior"),
                           no_germline_mode=no_germline_mode, device=device, het_beta=getattr(args, "het_beta", None))
    ratio = (getattr(args, GENOMIC_SPAN_NAME) - n) / n
    context = bool(getattr(args, "context_dependent_snv_priors", False))
    losses = model.learn_priors_and_spectra(rows, getattr(args, "num_spectrum_iterations"), ratio,
                                            learning_rate=getattr(args, "spectrum_learning_rate"), batch_size=POSTERIOR_BATCH_SIZE,
                                            context_dependent_snv_priors=context)
    thresholds = model.calculate_probability_thresholds(rows, germline_mode=germline_mode, recall_weight=getattr(args, "recall_weight"))
    out = posterior_outputs(model, rows, thresholds, losses, germline_mode)
    np.savez(getattr(args, "calls_output"), **out)
    log(f"posterior model: {n} candidates, {len(losses)} epochs in {time.perf_counter() - t0:.3f} s; thresholds "
        f"{ {v.name: round(float(t), 4) for v, t in thresholds.items()} }; {int(out['filtered_b'].sum())} filtered")
    if context and model.priors.last_context_fit is not None:
        log(f"context-dependent SNV priors: the last fit's largest |dF / d unknown| / max(sum k, 1) = {model.priors.last_context_fit_max_grad():.3e} "
            "(a deterministic estimator of the reference's model, not its ADVI fit)")
    if getattr(args, "evaluation_output", None):
        run_evaluation(args, posterior, rows, model, thresholds, out["filtered_b"], germline_mode, log)
    if getattr(args, "output_vcf", None):
        run_output_vcf(args, posterior, rows, out, germline_mode, device, vcf, log)
    return model, out


def run_output_vcf(args, posterior: MemoryMappedData, rows, out, germline_mode: bool, device, vcf=None, log=print):
    """--output_vcf: the input VCF with the filters and the five INFO fields of the calls just written (tools/filtered_vcf.py).  The
    filter decisions are the `filtered_b` of --calls_output, passed on."""
    import numpy as np
    from permutect_amd.enums import Call
    from permutect_amd.tools.filtered_vcf import write_filtered_vcf
    t0 = time.perf_counter()
    vcf = read_input_vcf(args) if vcf is None else vcf
    t1 = time.perf_counter()
    outputs = dict(out, artifact_logits_b=rows.artifact_logits.detach().float().cpu().numpy())
    int_rows = np.asarray(posterior.int_mmap[: posterior.num_data])
    counts = write_filtered_vcf(vcf.records, vcf.header, int_rows, outputs, Call.GERMLINE if germline_mode else Call.SOMATIC, device,
                                getattr(args, "output_vcf"))
    log(f"filtered VCF: {len(vcf.records)} lines, " + ", ".join(f"{name} {count}" for name, count in counts.items())
        + (f"; read {t1 - t0:.3f} s," if t1 - t0 > 1e-4 else ";") + f" match, plan and write {time.perf_counter() - t1:.3f} s")
    return counts


def run_evaluation(args, posterior: MemoryMappedData, rows, model, thresholds, filtered_b, germline_mode: bool, log=print):
    """--evaluation_output: the calls against the truth labels of the candidates (architecture/posterior_evaluation.py)"""
    from permutect_amd.architecture.posterior_evaluation import evaluate_against_truth, posterior_labels
    from permutect_amd.enums import Label, Variation
    t0 = time.perf_counter()
    labels_b = posterior_labels(posterior, device=rows.device)
    evaluation = evaluate_against_truth(model, rows, labels_b, thresholds, germline_mode=germline_mode,
                                        filtered_b=torch.from_numpy(filtered_b), keep_rows=True)
    evaluation.save(getattr(args, "evaluation_output"))
    labeled = evaluation.num_labeled()
    log(f"evaluation against truth: {labeled} labeled of {len(rows)} candidates, {evaluation.invalid} invalid, "
        f"{int(evaluation.mistakes.sum())} mistakes in {time.perf_counter() - t0:.3f} s"
        + ("" if labeled else "; no labeled candidates: the tables are empty"))
    sensitivity_v, precision_v = evaluation.sensitivity_precision()
    for v in Variation:
        c = evaluation.confusion[v]
        log(f"  {v.name}: variants {int(c[Label.VARIANT, 0])} passed / {int(c[Label.VARIANT, 1])} filtered, artifacts "
            f"{int(c[Label.ARTIFACT, 0])} passed / {int(c[Label.ARTIFACT, 1])} filtered, sensitivity {float(sensitivity_v[v]):.4f}, "
            f"precision {float(precision_v[v]):.4f} at threshold logit {float(evaluation.threshold_logits()[v]):.3f}")
    return evaluation


def parse_arguments(argv=None):
    parser = argparse.ArgumentParser(description="the artifact-model stage of filter_variants on an MI355X: candidates -> posterior data")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--" + TEST_DATASET_TAR_NAME, type=str, help="dataset tar (the reference's format) of the candidates")
    source.add_argument("--" + TEST_DATASET_NAME, type=str, help="Mutect2's plain-text dataset of the candidates, preprocessed in memory "
                        "(what preprocess_dataset would write to a tar)")
    parser.add_argument("--" + ARTIFACT_MODEL_NAME, type=str, required=True, help="artifact model from train_artifact_model (.pt, the reference's format)")
    parser.add_argument("--" + constants.OUTPUT_NAME, type=str, required=True, help="output tar of the posterior data")
    parser.add_argument("--" + constants.BATCH_SIZE_NAME, type=int, default=DEFAULT_BATCH_SIZE, required=False, help="batch size")
    parser.add_argument("--chunk_variants", type=int, default=None, required=False, help="candidates per HBM-resident chunk (default: the loader's)")
    # the site annotation (the reference's names); without --input nothing of it runs
    parser.add_argument("--" + constants.INPUT_NAME, type=str, default=None, required=False,
                        help="the Mutect2 VCF of the candidates: POPAF and the trusted filters are read from it (needs --contigs_table)")
    parser.add_argument("--" + CONTIGS_TABLE_NAME, type=str, default=None, required=False, help="table of `name index` lines: the dataset's contig indices")
    parser.add_argument("--" + MAF_SEGMENTS_NAME, type=str, default=None, required=False,
                        help="segments of the tumor's minor-allele fraction: contig, start, stop, maf (with --input)")
    parser.add_argument("--" + NORMAL_MAF_SEGMENTS_NAME, type=str, default=None, required=False,
                        help="segments of the normal's minor-allele fraction (with --input)")
    # the posterior stage (the reference's names and defaults, tools/filter_variants.py:83-163); without --genomic_span nothing of it runs
    parser.add_argument("--" + GENOMIC_SPAN_NAME, type=float, default=None, required=False,
                        help="number of sites considered by Mutect2, candidates or not: runs the posterior model behind the artifact model")
    parser.add_argument("--calls_output", type=str, default=None, required=False, help="output .npz of the posterior stage (with --genomic_span)")
    parser.add_argument("--num_spectrum_iterations", type=int, default=10, required=False, help="epochs of fitting the allele-fraction spectra")
    parser.add_argument("--spectrum_learning_rate", type=float, default=0.001, required=False, help="learning rate of that fit")
    parser.add_argument("--initial_log_variant_prior", type=float, default=-10.0, required=False, help="initial natural log prior of somatic variants")
    parser.add_argument("--initial_log_artifact_prior", type=float, default=-10.0, required=False, help="initial natural log prior of artifacts")
    parser.add_argument("--germline_mode", action="store_true", help="germline calls are not errors when the threshold is set")
    parser.add_argument("--no_germline_mode", action="store_true", help="no germline calls: somatic, artifact and sequencing error only")
    parser.add_argument("--het_beta", type=float, default=None, required=False, help="beta-binomial shape of the germline het spectrum instead of a binomial")
    parser.add_argument("--context_dependent_snv_priors", action="store_true",
                        help="learn the SNV prior per 3-base context and substitution in the second half of the epochs (a deterministic "
                             "estimator of the reference's model, not its ADVI fit)")
    parser.add_argument("--evaluation_output", type=str, default=None, required=False,
                        help="output .npz of the calls scored against the candidates' truth labels (with --genomic_span)")
    parser.add_argument("--output_vcf", type=str, default=None, required=False,
                        help="output path of the filtered VCF: --input with the filters and POST, PRIOR, SPECLL, ARTLOD, NORMLL of the calls "
                             "(with --input and --genomic_span; gzip when it ends in .gz)")
    parser.add_argument("--recall_weight", type=float, default=1.0, required=False, help="weight of recall against precision in the F-beta score")
    args = parser.parse_args(argv)
    if getattr(args, constants.INPUT_NAME) is not None and getattr(args, CONTIGS_TABLE_NAME) is None:
        parser.error(f"--{constants.INPUT_NAME} names candidates by contig name: it needs --{CONTIGS_TABLE_NAME}")
    for name in (MAF_SEGMENTS_NAME, NORMAL_MAF_SEGMENTS_NAME):
        if getattr(args, name) is not None and getattr(args, constants.INPUT_NAME) is None:
            parser.error(f"--{name} annotates the candidates of --{constants.INPUT_NAME}, which is missing")
    if posterior_stage_requested(args) and not args.calls_output:
        parser.error("--genomic_span runs the posterior stage, which needs --calls_output")
    if args.evaluation_output and not posterior_stage_requested(args):
        parser.error("--evaluation_output scores the posterior stage's calls, which needs --genomic_span")
    if args.output_vcf and getattr(args, constants.INPUT_NAME) is None:
        parser.error(f"--output_vcf rewrites the records of --{constants.INPUT_NAME}, which is missing")
    if args.output_vcf and not posterior_stage_requested(args):
        parser.error("--output_vcf writes the posterior stage's calls, which needs --genomic_span")
    return args


def main():
    main_without_parsing(parse_arguments())


if __name__ == "__main__":
    main()
