"""Downstream evaluation entry point (reference: /root/reference/eval.py).

    python eval.py experiment.target_dir=PATH [parameter.classifier={centroid,knn,kmeans,geometry,linear,nonlinear}]
                   [parameter.knn_k=200] [parameter.knn_t=0.1]
                   [parameter.kmeans_k=null] [parameter.kmeans_restarts=8] [parameter.kmeans_iters=50]
                   [+parameter.geometry_t=2.0]
                   [parameter.use_full_encoder=true]
"""
from simclr_amd.config import hydra_main
from simclr_amd.evaluation.features import evaluate


@hydra_main(config_path="conf", config_name="eval")
def main(cfg):
    return evaluate(cfg)


if __name__ == "__main__":
    main()
