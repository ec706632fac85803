"""Train BPRMF / NeuMF / SASRec / LightGCN / DirectAU / ComiRec / BUIR with the reference's demo flags (docs/demo_scripts_results/Topk_Amazon.sh:6,8,26,12,16,35,14) on the
Grocery split of tools/make_grocery_split.py through the plugin's main.py, in dense (torch.optim semantics) and
row-wise mode, and report test HR@5 / NDCG@5 next to the published numbers (docs/demo_scripts_results/README.md:47,48,56,49,51,57,50).
LightGCN, DirectAU, ComiRec and BUIR have no row-wise step (LightGCN's gradient is dense over L-hop neighbourhoods, DirectAU's
uniformity term couples every pair of the batch, ComiRec's model file has none yet, BUIR's target tables follow dense updates):
they run in dense mode only.
GPU box: python tools/run_grocery.py --out gpurun_out/<tag>/grocery_metrics.json"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rechorus_amd", "rechorus"))

PUBLISHED = {"BPRMF": (0.3549, 0.2486, 2.5), "NeuMF": (0.3237, 0.2221, 3.4), "SASRec": (0.3917, 0.2942, 5.5),
             "LightGCN": (0.3705, 0.2564, 6.1), "DirectAU": (0.3911, 0.2779, 3.3), "ComiRec": (0.3753, 0.2675, 4.5), "BUIR": (0.3701, 0.2567, 3.3),
             "FPMC": (0.3594, 0.2785, 3.4),      # (FPMC: not in the default --models list; Topk_Amazon.sh:18, README.md:52)
             "SLRCPlus": (0.4376, 0.3263, 4.3),  # (SLRCPlus: not in the default list either; needs item_meta.csv; README.md:62)
             "CFKG": (0.4199, 0.2984, 8.7)}      # (CFKG: not in the default list either; needs item_meta.csv; README.md:61)
FLAGS = {
    "BPRMF": ["--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6"],
    "NeuMF": ["--emb_size", "64", "--layers", "[64]", "--lr", "5e-4", "--l2", "1e-7", "--dropout", "0.2"],
    "SASRec": ["--emb_size", "64", "--num_layers", "1", "--num_heads", "1", "--lr", "1e-4", "--l2", "1e-6", "--history_max", "20"],
    "LightGCN": ["--emb_size", "64", "--n_layers", "3", "--lr", "1e-3", "--l2", "1e-8"],
    "DirectAU": ["--emb_size", "64", "--lr", "1e-3", "--l2", "1e-5", "--gamma", "0.3"],
    "ComiRec": ["--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6", "--attn_size", "8", "--K", "4", "--add_pos", "1", "--history_max", "20"],
    "BUIR": ["--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6"],
    "FPMC": ["--emb_size", "64", "--lr", "1e-3", "--l2", "1e-6", "--history_max", "20"],
    "SLRCPlus": ["--emb_size", "64", "--lr", "5e-4", "--l2", "1e-5", "--history_max", "20"],
    "CFKG": ["--emb_size", "64", "--margin", "1", "--include_attr", "1", "--lr", "1e-4", "--l2", "1e-6"],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--epoch", type=int, default=200)
    ap.add_argument("--models", default="BPRMF,NeuMF,SASRec,LightGCN,DirectAU,ComiRec,BUIR")
    ap.add_argument("--engines", default="dense,rowwise")
    a = ap.parse_args()
    import main as plugin_main
    data = os.path.join(ROOT, "data_local") + "/"
    if not os.path.exists(os.path.join(data, "Grocery_and_Gourmet_Food", "test.csv")):
        raise SystemExit("run tools/make_grocery_split.py in the build container first")
    res = {}
    for model in a.models.split(","):
        for engine in a.engines.split(","):
            if engine == "rowwise" and model in ("LightGCN", "DirectAU", "ComiRec", "BUIR"):
                continue
            if engine == "rowwise" and model == "NeuMF":
                extra = ["--dropout", "0.2"]
            else:
                extra = []
            log = f"/tmp/rc_grocery/{model}_{engine}.txt"
            t0 = time.perf_counter()
            try:
                out = plugin_main.run(["--model_name", model] + FLAGS[model] + extra + [
                    "--dataset", "Grocery_and_Gourmet_Food", "--path", data, "--epoch", str(a.epoch), "--engine", engine,
                    "--num_workers", "0", "--regenerate", "1" if engine == a.engines.split(",")[0] else "0", "--log_file", log,
                    "--model_path", f"/tmp/rc_grocery/{model}_{engine}.pt", "--save_final_results", "0"])
            except Exception as e:  # e.g. a configuration the row-wise step does not cover
                res[f"{model}/{engine}"] = {"error": str(e)[:300]}
                continue
            wall = time.perf_counter() - t0
            text = open(log).read()
            m = re.search(r"HR@5:([0-9.]+),NDCG@5:([0-9.]+)", out["test"])
            times = [float(x) for x in re.findall(r"\[([0-9.]+) s\]", text)]
            epochs = len(re.findall(r"Epoch \d+\s+loss=", text))
            pub = PUBLISHED[model]
            res[f"{model}/{engine}"] = {"test_HR@5": float(m.group(1)), "test_NDCG@5": float(m.group(2)), "epochs_run": epochs,
                                        "s_per_epoch_incl_eval": (sum(times[:epochs]) / max(epochs, 1)) if times else None,
                                        "wall_s": wall, "published_HR@5": pub[0], "published_NDCG@5": pub[1],
                                        "published_s_per_epoch": pub[2]}
            print(model, engine, res[f"{model}/{engine}"], flush=True)
    res["_note"] = ("dev/test regenerated from the bundled train.csv with the notebook's recipe (tools/make_grocery_split.py): "
                    "fewer training rows than upstream, so metrics are a ballpark check against the published table")
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
