"""makani_amd -- MI355X-native SFNO spectral stack (HIP kernels behind Makani's module API).

Mirrors the reference's interfaces for the hot path only:

* ``makani_amd.sht``                  RealSHT / InverseRealSHT (torch-harmonics seam)
* ``makani_amd.distributed``          DistributedRealSHT / DistributedInverseRealSHT, transposes
* ``makani_amd.spectral_convolution`` SpectralConv / FactorizedSpectralConv
* ``makani_amd.sfnonet``              FourierNeuralOperatorBlock / SphericalFourierNeuralOperatorNet
* ``makani_amd.afnonet``              AFNO2D / Block / AdaptiveFourierNeuralOperatorNet (block-diagonal spectral MLP kernels)
* ``makani_amd.afnonet_v1``           Mlp / AFNO2D / Block / AdaptiveFourierNeuralOperatorNet of the channels-last AFNOv1 (token <-> field
                                      layout passes around the planar transforms, block MLP with biases)
* ``makani_amd.vit``                  Attention / Block / VisionTransformer (scaled-dot-product attention on HIP MFMA kernels)
* ``makani_amd.comm``                 h / w / data process groups over torch.distributed (RCCL)
* ``makani_amd.preprocessor``         Preprocessor2D / get_preprocessor (one-pass HIP input assembly: ``assemble``)
* ``makani_amd.stepper``              SingleStepWrapper / MultiStepWrapper (the model wrappers of trainer and inferencer)
* ``makani_amd.inference``            Rollout (the inferencer's autoregressive rollout on a one-pass HIP step tail)
* ``makani_amd.stats``                DatasetStats (the statistics files of a dataset from one HIP pass per batch)
* ``makani_amd.histograms``           DatasetHistograms (per-channel value histograms, equal to np.histogram's, on one HIP pass)
* ``makani_amd.ensemble``             EnsembleScores (CRPS, spread, ensemble-mean RMSE and rank histogram per lead time, on one HIP pass;
                                      ``inference.EnsembleRollout`` runs and scores the perturbed members)
* ``makani_amd.grids``                GridConverter (equiangular -> Legendre-Gauss latitude interpolation of the loaders, with the
                                      loader's normalisation, on one HIP pass)
* ``makani_amd.noise``                SphericalNoise (isotropic Gaussian random fields with a prescribed spectrum, white or AR(1) in
                                      time, drawn into the packed spectrum on one HIP pass: the perturbation of ensemble members)

All arithmetic of the spectral path runs in libmakani_amd.so (include/makani_amd.h).
"""
__version__ = "0.1.0"
