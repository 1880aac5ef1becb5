! Capture wrapper for tests/golden/make_golden_dedd.py: bind(C) routines that set the module variables the delta-Eddington
! routines of the reference's ice_shortwave read, and call them on arrays handed in.  Compiled against the module files of
! the reference build (oracle/build_ref.sh, configuration small, or gx1 for --time) and of ice_shortwave and the four
! modules it uses, which the minter compiles from where they lie into its temporary directory; nothing of it is committed
! but this text.  The weights awt* are parameters of ice_constants in the stand-alone build and are not set here.
      module dedd_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine ddcap_set (tune_ice, tune_pnd, tune_snw) bind(C, name='ddcap_set')
      use ice_shortwave
      use ice_therm_vertical, only: heat_capacity
      real(c_double), value :: tune_ice, tune_pnd, tune_snw
      shortwave = 'dEdd'
      R_ice = tune_ice
      R_pnd = tune_pnd
      R_snw = tune_snw
      exp_min = exp(-10._dbl_kind)           ! init_dEdd's `exp_min = exp(-argmax)`
      heat_capacity = .true.
      end subroutine ddcap_set

      ! the value the reference's compiler gave exp_min (the minter holds it to the host libm's exp(-10))
      function ddcap_exp_min () result(v) bind(C, name='ddcap_exp_min')
      use ice_shortwave, only: exp_min
      real(c_double) :: v
      v = exp_min
      end function ddcap_exp_min

      ! shortwave_dEdd alone on one (block, category): fs, rhosnw, rsnw, fp, hp are the caller's
      subroutine ddcap_dedd (icells, indxi, indxj, coszen, aice, vice, vsno, fs, rhosnw, rsnw, fp, hp, swvdr, swvdf, &
                 swidr, swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, Sswabs, Iswabs, albice, albsno, albpnd) &
                 bind(C, name='ddcap_dedd')
      use ice_shortwave, only: shortwave_dEdd
      integer(c_int), value :: icells
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block)
      real(c_double), dimension(nx_block,ny_block) :: coszen, aice, vice, vsno, fs, fp, hp, swvdr, swvdf, swidr, swidf, &
         alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, albice, albsno, albpnd
      real(c_double) :: rhosnw(nx_block,ny_block,nslyr), rsnw(nx_block,ny_block,nslyr), Sswabs(nx_block,ny_block,nslyr), &
         Iswabs(nx_block,ny_block,nilyr)
      call shortwave_dEdd (nx_block, ny_block, icells, indxi, indxj, coszen, aice, vice, vsno, fs, rhosnw, rsnw, fp, hp, &
                           swvdr, swvdf, swidr, swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, Sswabs, &
                           Iswabs, albice, albsno, albpnd)
      end subroutine ddcap_dedd

      ! what step_radiation does for one (block, category) in its dEdd branch (ice_step_mod.F90:872-916): set_snow, set_pond
      ! (or, with_pond /= 0, fp and hp from the caller's apond, hpond), shortwave_dEdd
      subroutine ddcap_step (icells, indxi, indxj, with_pond, coszen, aice, vice, vsno, Tsfc, apond, hpond, swvdr, swvdf, &
                 swidr, swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, Sswabs, Iswabs, albice, albsno, albpnd) &
                 bind(C, name='ddcap_step')
      use ice_shortwave, only: shortwave_dEdd, shortwave_dEdd_set_snow, shortwave_dEdd_set_pond
      integer(c_int), value :: icells, with_pond
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block)
      real(c_double), dimension(nx_block,ny_block) :: coszen, aice, vice, vsno, Tsfc, apond, hpond, swvdr, swvdf, swidr, &
         swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, albice, albsno, albpnd
      real(c_double) :: Sswabs(nx_block,ny_block,nslyr), Iswabs(nx_block,ny_block,nilyr)
      real(dbl_kind), dimension(nx_block,ny_block) :: fsn, fpn, hpn
      real(dbl_kind), dimension(nx_block,ny_block,nslyr) :: rhosnwn, rsnwn
      call shortwave_dEdd_set_snow (nx_block, ny_block, icells, indxi, indxj, aice, vsno, Tsfc, fsn, rhosnwn, rsnwn)
      if (with_pond == 0) then
         call shortwave_dEdd_set_pond (nx_block, ny_block, icells, indxi, indxj, aice, Tsfc, fsn, fpn, hpn)
      else
         fpn(:,:) = apond(:,:)
         hpn(:,:) = hpond(:,:)
      endif
      call shortwave_dEdd (nx_block, ny_block, icells, indxi, indxj, coszen, aice, vice, vsno, fsn, rhosnwn, rsnwn, fpn, hpn, &
                           swvdr, swvdf, swidr, swidf, alvdr, alvdf, alidr, alidf, fswsfc, fswint, fswthru, Sswabs, &
                           Iswabs, albice, albsno, albpnd)
      end subroutine ddcap_step

      end module dedd_capture
