"""RealEstate10K novel-view-synthesis evaluation of the stitched decoder (the reference's evaluation/novel_view_synthesis_bench):
`re10k` reads the dataset, `nvs` renders held-out views, `metrics` scores them with the HIP SSIM / PSNR kernel and, given its weight
files, `lpips` (LPIPS(VGG)); `argument` is the command line of both scripts."""
